"""The inputs of tests/test_sketch_instances_gpu.py (helpers.sketch_case_*), checked on the CPU: each reaches the kernel
instantiation, tile seam or merge level it is built for.  A GPU test must not pass because its input quietly stopped reaching
the path, so what the cases claim is asserted here with the oracle and a Python restatement of the engine's plan
(helpers.sketch_plan, helpers.sketch_geometry -- plan_sketch_work in host_sketch.cpp, sketch_geometry in sketch.hip):

  wide      s in {2 049, 4 097, 12 288} is the NT = 1024 selector; the long record crosses a 28 672 seam and its sketch is full;
  geometry  each s of the boundary list lands on the NT and capacity it names, 12 289 on no LDS selector at all; sketches full;
  events    the -c stop falls between read 5 and read 799 for every k >= 4 in every mode;
  seams     the invalid byte or separator sits at TILE + d for every d in [-k, k], the sketches begin at all 16 alignments;
  slices    a sketch of one chunk of exactly four tiles, one of two chunks whose second holds a single k-mer start, offsets
            that are no multiples of four;
  merge     64 chunks (one level), 65 (32 + 32 + 1, one start in the last), 72 (ragged), the repeat seeded and short; the lone
            genome at the default plan is merged in two levels."""
import numpy as np
import pytest

from tests import helpers


def _plan_of(off, k, nt, env=None):
    return helpers.sketch_plan([int(x) for x in np.diff(off.astype(np.int64))], k, nt, env)


def test_sketch_geometry_rule():
    for s, want in helpers.SKETCH_GEOMETRY_SIZES.items():
        assert helpers.sketch_geometry(s) == want, s
    assert helpers.sketch_geometry(1) == (256, 4096) and helpers.sketch_geometry(1000) == (256, 4096)
    assert helpers.SKETCH_TILE == {256: 15360, 1024: 28672}
    for s in helpers.SKETCH_WIDE_SIZES + (3000,):
        assert helpers.sketch_geometry(s)[0] == 1024
    for s in (300, 1000):
        assert helpers.sketch_geometry(s)[0] == 256


def test_sketch_plan_restated():
    k, t = 21, 15360
    one = helpers.sketch_plan([4 * t + k - 1, 4 * t + k, k - 1, k, 20 * t], k, 256)
    assert one[0] == {"chunks": 1, "groups": [], "last": 4 * t} and one[1] == {"chunks": 2, "groups": [], "last": 1}
    assert one[2] is None and one[3] == {"chunks": 1, "groups": [], "last": 1} and one[4]["chunks"] == 5
    # a batch of many k-mers: chunks of total / 2 048, rounded up to tiles
    big = helpers.sketch_plan([2048 * 5 * t + k - 1], k, 256)
    assert big[0] == {"chunks": 2048, "groups": [32] * 64, "last": 5 * t}
    # one-tile chunks; the wide kernels round 15 360 up to their tile
    assert helpers.sketch_plan([3 * t + k], k, 256, helpers.SKETCH_ONE_TILE)[0] == {"chunks": 4, "groups": [], "last": 1}
    assert helpers.sketch_plan([2 * 28672 + k - 1], k, 1024, helpers.SKETCH_ONE_TILE)[0] == {"chunks": 2, "groups": [], "last": 28672}


@pytest.mark.parametrize("k", range(1, 33))
def test_wide_cases(oracle, k):
    case = helpers.sketch_case_wide(k)
    s = case["s"]
    assert helpers.sketch_geometry(s)[0] == 1024
    tile = helpers.SKETCH_TILE[1024]
    assert len(case["dna"][0][0]) > 2 * tile + k and len(case["protein"][0][0]) > (tile if s == 12288 else 0) + k
    for mode in (0, 1, 2):
        long_record = case["protein" if mode == 2 else "dna"][0]
        h = oracle.sketch_records(long_record, oracle.params(**dict(helpers.SKETCH_MODES[mode], k=k, s=s)))[0]
        if k >= (3 if mode == 2 else 6):
            assert len(h) == s, (k, mode, s, len(h))
        else:
            assert 0 < len(h) < s, (k, mode, s, len(h))      # fewer k-mers than s exist: the collection alone is exercised


def test_wide_cases_cover_every_size():
    assert {helpers.sketch_case_wide(k)["s"] for k in range(1, 33)} == set(helpers.SKETCH_WIDE_SIZES)
    for s in helpers.SKETCH_WIDE_SIZES:                       # each size at a k with 32-bit and at one with 64-bit hashes
        ks = [k for k in range(1, 33) if helpers.SKETCH_WIDE_SIZES[k % 3] == s]
        assert min(ks) <= 6 and any(6 <= k <= 16 for k in ks) and any(k > 16 for k in ks)


def test_geometry_cases(oracle):
    case = helpers.sketch_case_geometry()
    for kw, sketches in case.values():
        for s in helpers.SKETCH_GEOMETRY_SIZES:
            h = oracle.sketch_records(sketches[0], oracle.params(**dict(kw, s=s)))[0]
            assert len(h) == s, (kw, s)


@pytest.mark.parametrize("k", range(1, 33))
def test_event_cases_stop_inside_the_read_set(oracle, k):
    for mode in (0, 1, 2):
        reads = helpers.sketch_case_events(k, mode)
        assert len(reads) == helpers.SKETCH_EVENT_READS and min(map(len, reads)) >= 40 and max(map(len, reads)) <= 119
        kw = dict(helpers.SKETCH_MODES[mode], k=k, s=64)
        h, c, _, used, mult = oracle.sketch_reads(reads, oracle.params(**dict(kw, target_cov=helpers.SKETCH_EVENT_COV)))
        assert mult >= helpers.SKETCH_EVENT_COV
        if k >= 4:
            assert 5 <= used < helpers.SKETCH_EVENT_READS, (k, mode, used)
            assert len(h) == 64
        _, cb, _, _, _ = oracle.sketch_reads(reads, oracle.params(**dict(kw, target_cov=helpers.SKETCH_EVENT_COV, bloom_bytes=helpers.SKETCH_EVENT_BLOOM)))
        assert len(cb) and cb.min() >= 2                         # the filter admits a hash with count 2


@pytest.mark.parametrize("s", helpers.SKETCH_SEAM_SIZES)
@pytest.mark.parametrize("k", helpers.SKETCH_SEAM_KS)
def test_seam_cases(k, s):
    nt, _ = helpers.sketch_geometry(s)
    tile = helpers.SKETCH_TILE[nt]
    for mode in ((0, 1, 2) if k in helpers.SKETCH_SEAM_MODES else (0,)):
        kw, bases, off, where = helpers.sketch_case_seams(k, s, mode)
        n = len(off) - 1
        assert n == len(where) >= max(16, 2 * (2 * k + 1)) and n <= 130 and len(bases) < 8 << 20
        assert {int(o) % 16 for o in off[:-1]} == set(range(16))                    # every alignment of a tile's first 16-byte load
        assert {at - tile for at, _ in where} == set(range(-k, k + 1))
        invalid = {0: ord("N"), 2: ord("X")}.get(mode)
        for i, (at, byte) in enumerate(where):
            assert bases[int(off[i]) + at] == byte
            assert byte == 10 or (byte == invalid if mode != 1 else chr(byte) in "acgt")
        assert {byte == 10 for _, byte in where} == {False, True}
        lengths = np.diff(off.astype(np.int64))
        assert np.all(lengths == 2 * tile + 1001)
        as_is, cut = _plan_of(off, k, nt), _plan_of(off, k, nt, helpers.SKETCH_ONE_TILE)
        assert all(p["chunks"] == 1 for p in as_is) and all(p["chunks"] == 3 for p in cut)   # the tile seam is also a chunk seam
        assert kw.get("preserve_case", False) == (mode == 1)


@pytest.mark.parametrize("s", helpers.SKETCH_SEAM_SIZES)
def test_seam_cases_hold_kept_kmers_at_chunk_seams(oracle, s):
    """With chunks of one tile the k-mers that start at TILE and 2 TILE are the first of a chunk.  Some of them are kept hashes of
    their sketch (below its largest): a chunk that also emitted the start behind its end would count them twice."""
    k = 21
    nt, _ = helpers.sketch_geometry(s)
    tile = helpers.SKETCH_TILE[nt]
    kw, bases, off, _ = helpers.sketch_case_seams(k, s, 0)
    want = helpers.sketch_expected(oracle, kw, bases, off)
    raw = bases.tobytes()
    kept = 0
    for i, (h, c) in enumerate(want):
        for at in (tile, 2 * tile):
            one = oracle.sketch_records([raw[int(off[i]) + at: int(off[i]) + at + k]], oracle.params(**kw))[0]
            kept += len(one) == 1 and one[0] in h[:-1]
    assert kept >= 3, kept


@pytest.mark.parametrize("s", helpers.SKETCH_SEAM_SIZES)
@pytest.mark.parametrize("k", helpers.SKETCH_SLICE_KS)
def test_slice_cases(k, s):
    nt, _ = helpers.sketch_geometry(s)
    tile = helpers.SKETCH_TILE[nt]
    kw, bases, off = helpers.sketch_case_slices(k, s)
    assert len(bases) == int(off[-1]) and (nt == 256 or 395_000 < len(bases) < 410_000)
    assert b"\n" not in bases.tobytes() and set(bases.tobytes()) == set(b"ACGTN") and (bases == ord("N")).sum() == 3
    plan = _plan_of(off, k, nt)
    assert plan[0] is None and plan[1] is None and plan[2] == {"chunks": 1, "groups": [], "last": 1}
    assert plan[-2] == {"chunks": 1, "groups": [], "last": 4 * tile} and plan[-1] == {"chunks": 2, "groups": [], "last": 1}
    assert {int(o) % 4 for o in off} == {0, 1, 2, 3}                                 # packed input: offsets inside a byte of four bases


@pytest.mark.parametrize("nt", [256, 1024])
def test_merge_cases(oracle, nt):
    kw, bases, off, names = helpers.sketch_case_merge(nt)
    k, s = kw["k"], kw["s"]
    assert helpers.sketch_geometry(s)[0] == nt and len(bases) < 8 << 20
    plan = dict(zip(names, _plan_of(off, k, nt, helpers.SKETCH_ONE_TILE)))
    tile = helpers.SKETCH_TILE[nt]
    assert plan["c64"] == {"chunks": 64, "groups": [], "last": tile}
    assert plan["c65"] == {"chunks": 65, "groups": [32, 32, 1], "last": 1}
    assert plan["c72"] == {"chunks": 72, "groups": [32, 32, 8], "last": 5000}
    assert plan["repeat"]["chunks"] == 72 and plan["repeat"]["groups"] == [32, 32, 8]
    assert 1 < plan["plain"]["chunks"] <= 4 and plan["plain"]["groups"] == []
    want = dict(zip(names, helpers.sketch_expected(oracle, kw, bases, off)))
    for name in ("c64", "c65", "c72", "plain"):
        assert len(want[name][0]) == s
    # the repeat: seeded (3 s / npos < 1 / 4 of the hash range, 4^21 / 2 k-mers >> 64 npos) and short of s, so it is run again
    i = names.index("repeat")
    npos = int(off[i + 1] - off[i]) - k + 1
    assert 3.0 * s / npos < 0.25 and 4.0 ** k / 2 >= 64.0 * npos and len(want["repeat"][0]) == 700 < s
    assert want["repeat"][1].min() >= npos // 700


def test_merge_reads_and_genome_cases(oracle):
    kw, reads = helpers.sketch_case_merge_reads()
    k = kw["k"]
    total = sum(len(r) for r in reads) + len(reads) - 1
    plan = helpers.sketch_plan([total], k, 256, helpers.SKETCH_ONE_TILE)[0]
    assert plan["chunks"] > 140                                                       # the 72-chunk genome twice
    h, c, _, _, _ = oracle.sketch_records(reads, oracle.params(**kw))
    assert len(h) == kw["s"] and c.min() >= 2
    kw, genome = helpers.sketch_case_genome()
    plan = helpers.sketch_plan([len(genome)], kw["k"], 256)[0]
    assert len(genome) == 5_000_000 and plan["chunks"] == 82 and plan["groups"] == [32, 32, 18]     # chunks of four tiles: > 64
