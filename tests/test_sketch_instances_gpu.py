"""The sketch kernels (sketch.hip) at every instantiation, tile seam and merge level, against the CPU oracle.

sketch_chunks_kernel<K, MODE, NT, PROBE> is compiled for K = 1 .. 32, three modes and two workgroup sizes; count_chunks_kernel,
range_count_kernel and hash_events_kernel<K, MODE> for every K and mode.  The window dwords, the bytes a lane reads past its tile,
the lane stride, the tile and the LDS layout differ per (K, NT), so each is a kernel of its own that can be wrong alone.  The
inputs are helpers.sketch_case_* -- tests/test_sketch_cases_oracle.py asserts on the CPU that they reach what they are built for:

  1. the wide selector (NT = 1024, 2 048 < s <= 12 288) at every k in every mode, with multiplicities;
  2. the sketch sizes at which sketch_geometry changes the workgroup, the capacity or leaves the LDS selector;
  3. the event kernel of reads mode (-c, -b) at every k in every mode;
  4. an invalid byte and a record separator at every offset within k of a tile seam, at all 16 alignments of the tile's loads,
     the seam also as a chunk seam;
  5. sketches cut out of one buffer by offsets alone, at the lengths where a tile or a chunk ends; the packed path on the same;
  6. sketches of more than 64 chunks, merged in two levels, seeded and not, re-run, with min_copies, and a lone 5 Mbp genome;
  7. a reads session emptied by mg_reads_reset.

The judge is oracle.sketch_records / oracle.sketch_reads; hashes, nhash, multiplicities and reads used are compared exactly."""
import ctypes as C

import numpy as np
import pytest

from mash_amd import abi
from tests import helpers

pytestmark = pytest.mark.gpu

PAD = np.uint64(abi.HASH_PAD)
OTHER_ENV = ("MASHGPU_PACKED_PIECE", "MASHGPU_PACKED_UNPACK", "MASHGPU_MINCOPIES_EXPECT")


@pytest.fixture(scope="module")
def eng():
    import torch
    torch.cuda.init()          # (torch ships its own HIP runtime: it initialises first, tests/test_gpu_parity.py)
    e = abi.MashGpu(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def judged(oracle):
    """key, builder -> what the builder returns (a case and the oracle's rows of it): computed once, shared by the variants of a test"""
    done = {}

    def get(key, build):
        if key not in done:
            done[key] = build()
        return done[key]
    return get


def _set_env(monkeypatch, one_tile=False, no_seed=False):
    for v in helpers.SKETCH_ENV + OTHER_ENV:
        monkeypatch.delenv(v, raising=False)
    if one_tile:
        for v, x in helpers.SKETCH_ONE_TILE.items():
            monkeypatch.setenv(v, x)
    if no_seed:
        monkeypatch.setenv("MASHGPU_SKETCH_NO_SEED", "1")


def _check_rows(got, want, s, what):
    """every row: nhash, the hashes, the padding behind them, the multiplicities and zeros behind them"""
    hashes, nhash, counts = got
    assert hashes.shape == (len(want), s) and counts.shape == (len(want), s), what
    for i, (h, c) in enumerate(want):
        n = len(h)
        assert nhash[i] == n, (what, i, int(nhash[i]), n)
        bad = np.nonzero(hashes[i, :n] != h)[0]
        assert len(bad) == 0, (what, i, "%d of %d hashes differ, first at %d" % (len(bad), n, bad[0]))
        assert np.all(hashes[i, n:] == PAD), (what, i)
        bad = np.nonzero(counts[i, :n] != c)[0]
        assert len(bad) == 0, (what, i, "%d of %d counts differ, first at %d: got %d, expected %d" % (
            len(bad), n, bad[0] if len(bad) else 0, counts[i, bad[0]] if len(bad) else 0, c[bad[0]] if len(bad) else 0))
        assert not counts[i, n:].any(), (what, i)


def _oracle_rows(oracle, kw, sketches):
    p = oracle.params(**kw)
    return [oracle.sketch_records(list(recs), p)[:2] for recs in sketches]


# ---------------------------------------------------------------------------------------------- 1. the wide selector

@pytest.mark.parametrize("k", range(1, 33))
def test_wide_selector_every_instantiation(eng, oracle, k, monkeypatch):
    """sketch_chunks_kernel<k, MODE, 1024> for the three modes, s cycling over 2 049 (the first size of the wide kernels), 4 097
    (the first of the 16 384 buffer) and 12 288 (the last of the selector; in MODE 2 the alphabet table then sits behind 128 KB
    of candidates): a record with seams of the 28 672 tile and adversarial records; count_chunks_kernel<k, MODE> walks the same
    plan, cut for the wide tile, with its own tile of 15 360."""
    _set_env(monkeypatch)
    case = helpers.sketch_case_wide(k)
    s = case["s"]
    for mode in (0, 1, 2):
        kw = dict(helpers.SKETCH_MODES[mode], k=k, s=s)
        sketches = case["protein" if mode == 2 else "dna"]
        want = _oracle_rows(oracle, kw, sketches)
        _check_rows(eng.sketch_host(sketches, eng.params(**kw), counts=True), want, s, (k, mode, s))
        if k >= (3 if mode == 2 else 6):
            assert len(want[0][0]) == s                                 # the selection, not just the collection


# ---------------------------------------------------------------------------------------------- 2. the boundaries of the geometry

@pytest.mark.parametrize("s", list(helpers.SKETCH_GEOMETRY_SIZES))
@pytest.mark.parametrize("which", ["dna", "protein"])
def test_geometry_boundaries(eng, oracle, which, s, monkeypatch):
    """s = 2 048 | 2 049: NT 256 -> 1024; 4 096 | 4 097: capacity 8 192 -> 16 384; 12 288 | 12 289: the LDS selector -> range
    counting in HBM.  Canonical 21-mers of 150 kbp and protein 9-mers of 40 000 residues, full sketches, with multiplicities."""
    _set_env(monkeypatch)
    kw, sketches = helpers.sketch_case_geometry()[which]
    kw = dict(kw, s=s)
    want = _oracle_rows(oracle, kw, sketches)
    assert len(want[0][0]) == s
    _check_rows(eng.sketch_host(sketches, eng.params(**kw), counts=True), want, s, (which, s))


# ---------------------------------------------------------------------------------------------- 3. the event kernel

@pytest.mark.parametrize("k", range(1, 33))
def test_event_kernel_every_instantiation(eng, oracle, k):
    """hash_events_kernel<k, MODE> for the three modes: 800 reads with -c 3 in one call and through a session 37 reads at a time,
    and with -b 700 on top.  Hashes, counts and reads used are the oracle's; for k >= 4 the stop lies inside the read set, so the
    positions of the events decide after which read the input ends."""
    for mode in (0, 1, 2):
        reads = helpers.sketch_case_events(k, mode)
        kw = dict(helpers.SKETCH_MODES[mode], k=k, s=64, target_cov=helpers.SKETCH_EVENT_COV)
        oh, oc, _, oused, _ = oracle.sketch_reads(reads, oracle.params(**kw))
        if k >= 4:
            assert 5 <= oused < helpers.SKETCH_EVENT_READS, (k, mode, oused)
        p = eng.params(**kw)
        h, c, used = eng.sketch_reads(reads, p)
        assert used == oused and np.array_equal(h, oh) and np.array_equal(c, oc), (k, mode, used, oused)
        h, c, used, fed = eng.sketch_reads_chunked(reads, p, 37)
        assert used == oused and np.array_equal(h, oh) and np.array_equal(c, oc), (k, mode, "chunked", used, oused)
        assert fed == (oused + 36) // 37, (k, mode, fed, oused)                   # (no read of these is shorter than k)
        kw["bloom_bytes"] = helpers.SKETCH_EVENT_BLOOM
        oh, oc, _, oused, _ = oracle.sketch_reads(reads, oracle.params(**kw))
        h, c, used = eng.sketch_reads(reads, eng.params(**kw))
        assert used == oused and np.array_equal(h, oh) and np.array_equal(c, oc), (k, mode, "bloom", used, oused)


# ---------------------------------------------------------------------------------------------- 4. tile and chunk seams

@pytest.mark.parametrize("s", helpers.SKETCH_SEAM_SIZES)
@pytest.mark.parametrize("k", helpers.SKETCH_SEAM_KS)
def test_seam_sweep(eng, oracle, judged, k, s, monkeypatch):
    """A lane's run reads k - 1 bytes past its tile and `remaining` cuts what it may emit.  For every d in [-k, k]: an invalid
    byte at TILE + d (it voids the k-mers that hold it, on both sides of the seam) and a record separator there (the same, and
    the oracle starts a new record), the sketches beginning at all 16 alignments (shift, bsh).  Each batch as the plan cuts it
    (one chunk per sketch) and in chunks of one tile: the same seam between two workgroups that share a threshold."""
    for mode in ((0, 1, 2) if k in helpers.SKETCH_SEAM_MODES else (0,)):
        def build():
            kw, bases, off, where = helpers.sketch_case_seams(k, s, mode)
            return kw, bases, off, helpers.sketch_expected(oracle, kw, bases, off)
        kw, bases, off, want = judged(("seams", k, s, mode), build)
        assert {int(o) % 16 for o in off[:-1]} == set(range(16))
        p = eng.params(**kw)
        seen = []
        for one_tile in (False, True):
            _set_env(monkeypatch, one_tile)
            got = eng.sketch_host_raw(bases, off, p, counts=True)
            _check_rows(got, want, s, (k, s, mode, one_tile))
            seen.append(b"".join(a.tobytes() for a in got))
        assert seen[0] == seen[1]


# ---------------------------------------------------------------------------------------------- 5. slices of one genome

@pytest.mark.parametrize("s", helpers.SKETCH_SEAM_SIZES)
@pytest.mark.parametrize("k", helpers.SKETCH_SLICE_KS)
def test_slices_of_one_genome(eng, oracle, k, s, monkeypatch):
    """One buffer without a separator, cut by off[] into slices of 0, k - 1, k, k + 1, 15 .. 17, T - 1 .. T + k and 4 T + k - 1 | 4 T + k
    bytes (one chunk | two, the second of a single k-mer start): each row is the oracle's sketch of its slice alone, so no k-mer
    leaks across `limit`.  The packed path (the kernel expanding two-bit codes while it stages a tile) gives the same bytes from
    offsets that are no multiples of four, with a mask, as one piece and in pieces of 4 000 bases."""
    _set_env(monkeypatch)
    kw, bases, off = helpers.sketch_case_slices(k, s)
    want = helpers.sketch_expected(oracle, kw, bases, off)
    p = eng.params(**kw)
    got = eng.sketch_host_raw(bases, off, p, counts=True)
    _check_rows(got, want, s, (k, s))
    assert not got[1][:2].any() and got[1][2] == 1                       # shorter than k: empty; exactly k bytes: one k-mer
    packed, mask, ninv = abi.pack_bases(bases)
    assert ninv == 3 and mask.any() and {int(o) % 4 for o in off} == {0, 1, 2, 3}
    for piece in (None, "4000"):
        if piece:
            monkeypatch.setenv("MASHGPU_PACKED_PIECE", piece)
        h, n = eng.sketch_host_packed_raw(packed, mask, len(bases), off, p)
        assert np.array_equal(n, got[1]), (k, s, piece)
        assert h.tobytes() == got[0].tobytes(), (k, s, piece, np.argwhere(h != got[0])[:5])


# ---------------------------------------------------------------------------------------------- 6. the two-level merge

@pytest.mark.parametrize("nt", [256, 1024])
def test_two_level_merge(eng, oracle, nt, monkeypatch):
    """Chunks of one tile.  64 chunks: one merge.  65: groups of 32, 32 and 1 slot are merged into their first slot (to_pool), then
    the three group results (stride 32); the last chunk is a single k-mer start.  72: a ragged last group of 8.  The 700-base unit
    repeated over 72 chunks is seeded, comes out with 700 hashes and is run again (rerun_short_sketches replays both levels).
    Seeded and unseeded give the oracle's rows and the same bytes."""
    kw, bases, off, names = helpers.sketch_case_merge(nt)
    want = helpers.sketch_expected(oracle, kw, bases, off)
    assert len(want[names.index("repeat")][0]) == 700
    p = eng.params(**kw)
    seen = []
    for no_seed in (False, True):
        _set_env(monkeypatch, one_tile=True, no_seed=no_seed)
        got = eng.sketch_host_raw(bases, off, p, counts=True)
        _check_rows(got, want, kw["s"], (nt, names, no_seed))
        seen.append(b"".join(a.tobytes() for a in got))
    assert seen[0] == seen[1]


def test_many_chunks_with_min_copies(eng, oracle, monkeypatch):
    """The 72-chunk genome as overlapping reads that cover it twice, min_copies = 2: range_count_kernel over more than 140 chunks
    of one tile; hashes and multiplicities."""
    _set_env(monkeypatch, one_tile=True)
    kw, reads = helpers.sketch_case_merge_reads()
    want = _oracle_rows(oracle, kw, [reads])
    assert len(want[0][0]) == kw["s"]
    _check_rows(eng.sketch_host([reads], eng.params(**kw), counts=True), want, kw["s"], "min_copies")


def test_lone_genome_at_the_default_plan(eng, oracle, monkeypatch):
    """`mash sketch genome.fna` of one bacterial genome: a single record of 5 Mbp is 82 chunks of four tiles, merged in groups of
    32, 32 and 18 and then once more; nothing about the plan is set."""
    _set_env(monkeypatch)
    kw, genome = helpers.sketch_case_genome()
    want = _oracle_rows(oracle, kw, [[genome]])
    assert len(want[0][0]) == kw["s"]
    _check_rows(eng.sketch_host([[genome]], eng.params(**kw), counts=True), want, kw["s"], "genome")


# ---------------------------------------------------------------------------------------------- 7. mg_reads_reset

class _ReadsSession:
    """mg_reads_begin .. mg_reads_free with what abi.MashGpu.sketch_reads_chunked does not hand out: whether an add stopped"""

    def __init__(self, eng, p):
        self.eng, self.p, self.h = eng, p, C.c_void_p()
        eng._check(eng.lib.mg_reads_begin(eng.ctx, C.byref(p), C.byref(self.h)))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.eng.lib.mg_reads_free(self.h)

    def add(self, records):
        blob = np.frombuffer(abi.join_records(records) + bytes([abi.RECORD_SEP]), dtype=np.uint8)
        stopped = C.c_int(0)
        self.eng._check(self.eng.lib.mg_reads_add_host(self.h, blob.ctypes.data, len(blob), C.byref(stopped)))
        return bool(stopped.value)

    def feed(self, records, per=37):
        for o in range(0, len(records), per):
            if self.add(records[o:o + per]):
                return True
        return False

    def reset(self):
        self.eng._check(self.eng.lib.mg_reads_reset(self.h))

    def finish(self):
        s = int(self.p.sketch_size)
        hashes, counts = np.full(s, PAD, dtype=np.uint64), np.zeros(s, dtype=np.uint32)
        n, used = C.c_uint32(0), C.c_uint64(0)
        self.eng._check(self.eng.lib.mg_reads_finish(self.h, hashes.ctypes.data, C.byref(n), counts.ctypes.data, C.byref(used)))
        return hashes[: n.value].copy(), counts[: n.value].copy(), int(used.value)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


@pytest.mark.parametrize("option", ["target_cov", "bloom_bytes"])
def test_reads_session_reset_leaves_no_trace(eng, oracle, option):
    """A session that has stopped on -c, and one whose -b filter is full of another read set's bits, emptied by mg_reads_reset:
    the next read set gives what a fresh session gives and what the oracle gives -- heap, filter, stop and the count of reads
    all start over."""
    kw = {"k": 21, "s": 64}
    kw.update({"target_cov": helpers.SKETCH_EVENT_COV} if option == "target_cov" else {"bloom_bytes": helpers.SKETCH_EVENT_BLOOM})
    first, second = helpers.sketch_case_events(21, 0), helpers.sketch_case_events(22, 0)
    p = eng.params(**kw)
    want = []
    for reads in (first, second):
        oh, oc, _, oused, _ = oracle.sketch_reads(reads, oracle.params(**kw))
        want.append((oh, oc, oused))
    assert not np.array_equal(want[0][0], want[1][0])
    with _ReadsSession(eng, p) as fresh:
        fresh.feed(second)
        alone = fresh.finish()
    assert _same(alone, want[1])
    with _ReadsSession(eng, p) as rs:
        stopped = rs.add(first)                                          # one chunk: the stop falls inside it
        assert stopped == (option == "target_cov")
        assert _same(rs.finish(), want[0])
        if stopped:
            assert rs.add(second[:5]) and _same(rs.finish(), want[0])    # a stopped session takes nothing more
        rs.reset()
        assert rs.finish()[2] == 0 and len(rs.finish()[0]) == 0
        assert rs.feed(second) == (option == "target_cov")
        assert _same(rs.finish(), alone)
        rs.reset()                                                       # and once more, the first set again
        rs.feed(first, per=211)
        assert _same(rs.finish(), want[0])
