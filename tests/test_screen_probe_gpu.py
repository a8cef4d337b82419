"""`mash screen`'s probe on the paths of the sketch kernel it is fused into (sketch_chunks_kernel<.., PROBE = true>, sketch.hip).

An observation count is right only if every path of that kernel looks each k-mer up exactly once.  Two paths exist to keep it
from happening twice: a steady tile that overflows the candidate buffer is run again with the probe off, and a seeded batch
whose sketch came out short is run again whole with the probe off (rerun_short_sketches, host_sketch.cpp).  The cases of
tests/helpers.py (screen_case_*) reach them -- tests/test_screen_probe_oracle.py asserts on the CPU that they do -- next to sketch
sizes above 2 048 (the NT = 1024 kernels), other hash seeds, forward-only and translated k-mers, one-tile chunks, one chunk per
batch and MASHGPU_SKETCH_NO_SEED.

The judge is helpers.screen_expected: every valid k-mer of the mixture hashed by the oracle and counted.  Every test compares
counts[i, :nhash[i]] of EVERY database row and the mixture sketch with it, exactly."""
import numpy as np
import pytest

from mash_amd import abi
from tests import helpers

pytestmark = pytest.mark.gpu

# how the batch is cut into chunks (plan_sketch_work, host_sketch.cpp): its own choice (chunks of four tiles here), chunks of one
# tile (15 360 is rounded up to the tile of the wide kernels), one chunk per batch
CHUNKING = {"default": {}, "one_tile": {"MASHGPU_SKETCH_MIN_CHUNK": "15360", "MASHGPU_SKETCH_ITEMS": "100000"},
            "one_chunk": {"MASHGPU_SKETCH_ITEMS": "1"}}
SKETCH_ENV = ("MASHGPU_SKETCH_MIN_CHUNK", "MASHGPU_SKETCH_ITEMS", "MASHGPU_SKETCH_NO_SEED", "MASHGPU_SKETCH_SEED_FACTOR")


@pytest.fixture(scope="module")
def eng():
    import torch
    torch.cuda.init()          # (torch ships its own HIP runtime: it initialises first, tests/test_gpu_parity.py)
    e = abi.MashGpu(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def judged(oracle):
    """name -> (case, (table, nhash, lengths), expected rows, expected mixture sketch); each computed once, read-only"""
    done = {}

    def get(name):
        if name not in done:
            case = helpers.screen_case(name)
            db = helpers.screen_db(oracle, case)
            counts, mix = helpers.screen_expected(oracle, case["params"], case["batches"], case["translate"])
            rows = helpers.screen_expected_rows(counts, db[0], db[1])
            for a in db + (rows, mix):
                a.flags.writeable = False
            done[name] = (case, db, rows, mix)
        return done[name]
    return get


def _set_sketch_env(monkeypatch, chunking="default", no_seed=False):
    for v in SKETCH_ENV:
        monkeypatch.delenv(v, raising=False)
    for v, x in CHUNKING[chunking].items():
        monkeypatch.setenv(v, x)
    if no_seed:
        monkeypatch.setenv("MASHGPU_SKETCH_NO_SEED", "1")


def _screen(eng, case, db, batches):
    table, nhash, lengths = db
    t = eng.table_upload(table, nhash, lengths)
    try:
        with eng.screen_open(t, eng.params(**case["params"]), translate=case["translate"]) as sc:
            for recs in batches:
                sc.add_host(helpers.screen_blob(recs))
            return sc.finish()
    finally:
        t.free()


def _check(got, db, rows, mix):
    """counts of every row, the cells behind a row's nhash, the mixture sketch and the number of distinct keys, exactly"""
    counts, got_mix, distinct = got
    table, nhash, _ = db
    assert counts.shape == rows.shape and counts.dtype == np.uint32
    for i in range(len(nhash)):
        n = int(nhash[i])
        bad = np.nonzero(counts[i, :n] != rows[i, :n])[0]
        assert len(bad) == 0, "row %d: %d of %d counts differ, first at hash %d: got %d, expected %d" % (
            i, len(bad), n, table[i, bad[0]], counts[i, bad[0]], rows[i, bad[0]])
        assert not counts[i, n:].any(), i
    assert np.array_equal(got_mix, mix)
    assert distinct == len(np.unique(table[table != helpers.PAD]))


_seen = {}          # case -> the bytes of its first variant: every variant gives the same


def _same_as_the_other_variants(name, got):
    b = (got[0].tobytes(), got[1].tobytes())
    assert _seen.setdefault(name, b) == b


@pytest.mark.parametrize("no_seed", [False, True], ids=["seeded", "no_seed"])
@pytest.mark.parametrize("chunking", list(CHUNKING))
@pytest.mark.parametrize("name", ["flood", "flood_wide", "flood_forward", "flood_translated"])
def test_screen_flooded_tiles_are_probed_once(eng, judged, name, chunking, no_seed, monkeypatch):
    """Runs of one k-mer that is a database key and lies inside the batch's sketch: whole steady tiles overflow the candidate buffer
    and are run again.  flood: canonical 21-mers, s = 1000 (the T run counts on the A run's key; a tandem repeat of a 23-mer takes
    the segmented path beside it); flood_wide: s = 3000, the NT = 1024 kernels; flood_forward: MODE 1, 32-bit hashes, two keys;
    flood_translated: a run of K in the three forward frames of 150 000 A.  A tile probed twice doubles the runs' counts.
    (One variant cannot overflow: unseeded, a one-tile chunk inside the run starts without a threshold, so its only tile takes the
    segmented pass.  It is here for its bytes, which must be those of the others.)"""
    case, db, rows, mix = judged(name)
    _set_sketch_env(monkeypatch, chunking, no_seed)
    got = _screen(eng, case, db, case["batches"])
    _check(got, db, rows, mix)
    _same_as_the_other_variants(name, got)


@pytest.mark.parametrize("no_seed", [False, True], ids=["seeded", "no_seed"])
@pytest.mark.parametrize("chunking", ["default", "one_tile"])
def test_screen_short_batches_are_probed_once(eng, judged, chunking, no_seed, monkeypatch):
    """A batch of 400 copies of a 700-base unit (fewer than s distinct k-mers) and one of 120 copies of a 2 500-base unit (next to
    none of its hashes below the seeded threshold) come out short and are run again without a seed; the rows of the two units
    count 399 or 400 and 119 or 120 -- twice that if the second run probed again.  Unseeded, nothing is run again: same bytes."""
    case, db, rows, mix = judged("short")
    _set_sketch_env(monkeypatch, chunking, no_seed)
    got = _screen(eng, case, db, case["batches"])
    _check(got, db, rows, mix)
    _same_as_the_other_variants("short", got)


def test_screen_resident_session_with_a_flooded_key(eng, judged, monkeypatch):
    """The flood mixture through one session: the sparse hits are the non-zero cells of the dense counts (the flooded key once per
    row that holds it), a reset clears the flooded counter through the touched list, the mixture added again gives the same bytes;
    without the key tiers the same counts."""
    case, db, rows, mix = judged("flood")
    table, nhash, lengths = db
    _set_sketch_env(monkeypatch)
    p = eng.params(**case["params"])
    t = eng.table_upload(table, nhash, lengths)

    def add_all(sc):
        for recs in case["batches"]:
            sc.add_host(helpers.screen_blob(recs))

    with eng.screen_open(t, p) as sc:
        add_all(sc)
        first = sc.finish()
        hits, hmix, hdistinct = sc.finish_sparse()
        _check(first, db, rows, mix)
        helpers.hits_equal_counts(hits, first[0], table, nhash)
        assert np.array_equal(hmix, mix) and hdistinct == first[2]
        flooded = hits[hits["hash"] == table[0, 0]]
        assert flooded["row"].tolist() == [0, 1, 2] and flooded["count"].tolist() == [int(rows[0, 0])] * 3
        sc.reset()
        none, mix0, _ = sc.finish_sparse()
        assert len(none) == 0 and len(mix0) == 0
        zero, mix0, _ = sc.finish()
        assert not zero.any() and len(mix0) == 0
        add_all(sc)
        again = sc.finish()
        hits2, _, _ = sc.finish_sparse()
        assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()
        assert hits2.tobytes() == hits.tobytes()
    monkeypatch.setenv("MASHGPU_SCREEN_TIERS", "0")
    with eng.screen_open(t, p) as sc:
        assert "off" in sc.tier_note(), sc.tier_note()
        add_all(sc)
        one_tier = sc.finish()
    _check(one_tier, db, rows, mix)
    t.free()


def test_screen_batch_edges(eng, oracle, judged, monkeypatch):
    """Batches at the edges of the batch format (helpers.screen_case_batch_edges); the same bytes from device memory; a device
    pointer that is not 16-byte aligned is refused and the session goes on."""
    import torch
    case, db, rows, mix = judged("batch_edges")
    table, nhash, lengths = db
    batches = case["batches"]
    _set_sketch_env(monkeypatch)
    p = eng.params(**case["params"])
    t = eng.table_upload(table, nhash, lengths)
    with eng.screen_open(t, p) as sc:
        sc.add_host(helpers.screen_blob(batches[0]))                          # shorter than k: nothing
        counts, got_mix, _ = sc.finish()
        assert not counts.any() and len(got_mix) == 0
        sc.add_host(helpers.screen_blob(batches[1]))                          # exactly k bytes: one k-mer, the key of rows 0 .. 2
        counts, got_mix, _ = sc.finish()
        assert counts[:3, 0].tolist() == [1, 1, 1] and counts.sum() == 3 and got_mix.tolist() == [int(table[0, 0])]
        for recs in batches[2:]:
            sc.add_host(helpers.screen_blob(recs))
        host = sc.finish()
    _check(host, db, rows, mix)
    # ---- the same joined bytes from 16-byte aligned device memory
    bufs = [torch.from_numpy(helpers.screen_blob(recs).copy()).cuda() for recs in batches]
    torch.cuda.synchronize()
    with eng.screen_open(t, p) as sc:
        for b in bufs:
            assert b.numel() == 0 or b.data_ptr() % 16 == 0
            sc.add_dev(b.data_ptr(), b.numel())
        dev = sc.finish()
    assert dev[0].tobytes() == host[0].tobytes() and dev[1].tobytes() == host[1].tobytes()
    # ---- a pointer off by one byte: an error, and the session stays usable
    part = [batches[3], batches[4]]
    want, want_mix = helpers.screen_expected(oracle, case["params"], part)
    with eng.screen_open(t, p) as sc:
        sc.add_host(helpers.screen_blob(part[0]))
        with pytest.raises(abi.MashGpuError, match="16-byte aligned"):
            sc.add_dev(bufs[4].data_ptr() + 1, bufs[4].numel() - 1)
        sc.add_host(helpers.screen_blob(part[1]))
        _check(sc.finish(), db, helpers.screen_expected_rows(want, table, nhash), want_mix)
    t.free()
