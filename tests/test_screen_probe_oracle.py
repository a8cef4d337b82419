"""The judge of tests/test_screen_probe_gpu.py, checked on the CPU: helpers.screen_expected (every valid k-mer of the mixture hashed
by the oracle and counted) against a second computation, the per-record sum of sketch_records([record], s > the record's k-mers)
counts that the older screen tests use as truth -- with the oracle and, where it is built, with the reference's own MinHashHeap.  Then the
conditions that make the GPU tests reach the two paths of the fused sketch + probe kernel that keep a k-mer from being looked up
twice, on the oracle's output alone:

  flood   a run of one k-mer whose hash is a database key and lies inside the batch's own sketch, at least three tiles long: at
          least one whole tile lies inside the run, every one of its k-mers passes h < T, they are more than the candidate buffer
          holds (cap <= 4 096 for s <= 2 048, <= 16 384 above), so a steady tile overflows and is run again;
  short   a batch that seed_thresholds (host_sketch.cpp) seeds and whose sketch then has fewer than s hashes below the seed: the
          whole batch is run again without one.
"""
import numpy as np
import pytest

from tests import helpers

# k-mer starts per tile of sketch_chunks_kernel: NT * sk_L(NT) (sk_L in kmer_stream.h), NT chosen by sketch_geometry (sketch.hip):
# 256 lanes of 60 starts while s + 2 048 fits a buffer of 16 hashes per lane (s <= 2 048), 1 024 lanes of 28 up to s = 12 288
TILE_SMALL, TILE_WIDE = 256 * 60, 1024 * 28
S_SMALL_MAX = 2048


@pytest.fixture(scope="module")
def screen_cases(oracle):
    """name -> (case, (table, nhash, lengths), counts, mix, expected rows); computed once, read-only"""
    out = {}
    for name in helpers.SCREEN_CASES:
        case = helpers.screen_case(name)
        db = helpers.screen_db(oracle, case)
        counts, mix = helpers.screen_expected(oracle, case["params"], case["batches"], case["translate"])
        rows = helpers.screen_expected_rows(counts, db[0], db[1])
        for a in db + (mix, rows):
            a.flags.writeable = False
        out[name] = (case, db, counts, mix, rows)
    return out


def test_screen_expected_on_a_mixture_counted_by_hand(oracle):
    kw = {"k": 3, "s": 2, "noncanonical": True}
    counts, mix = helpers.screen_expected(oracle, kw, [[b"ACGTACG", b"AC"], [b"", b"acgNACG"]])
    h = lambda kmer: oracle.get_hash(kmer, 42, False)                       # 4^3 k-mers: 32-bit hashes
    assert counts == {h(b"ACG"): 4, h(b"CGT"): 1, h(b"GTA"): 1, h(b"TAC"): 1}       # (a k-mer with an N is none; lower case is folded)
    assert list(mix) == sorted(counts)[:2]
    both, _ = helpers.screen_expected(oracle, {"k": 3, "s": 2}, [[b"ACG", b"CGT"]])  # canonical: a k-mer and its reverse complement
    assert list(both.values()) == [2]
    empty, none = helpers.screen_expected(oracle, kw, [])
    assert empty == {} and len(none) == 0
    table = np.array([[h(b"ACG"), h(b"TAC")], [h(b"TTT"), helpers.PAD]], dtype=np.uint64)
    assert helpers.screen_expected_rows(counts, table, np.array([2, 1])).tolist() == [[4, 1], [0, 0]]


@pytest.mark.parametrize("which", ["oracle", "ref_oracle"])
@pytest.mark.parametrize("name", helpers.SCREEN_CASES)
def test_screen_expected_equals_the_sum_over_single_records(request, screen_cases, name, which):
    orc = request.getfixturevalue(which)                                    # (ref_oracle: the reference's own MinHashHeap)
    case, _, counts, mix, _ = screen_cases[name]
    kw = case["params"]
    params = {}                                                             # per record length: a sketch size no record can fill,
    want = {}                                                               # so its sketch is every distinct hash with its count
    for recs in case["batches"]:
        for r in recs:
            for x in (orc.six_frames(r) if case["translate"] else [r]):
                if len(x) < kw["k"]:
                    continue
                if len(x) not in params:
                    params[len(x)] = orc.params(**dict(kw, s=len(x) + 1))
                h, c, _, _, _ = orc.sketch_records([x], params[len(x)])
                assert len(h) <= len(x) - kw["k"] + 1
                for hv, cv in zip(h.tolist(), c.tolist()):
                    want[hv] = want.get(hv, 0) + cv
    assert counts == want
    assert np.array_equal(mix, np.array(sorted(want), dtype=np.uint64)[: case["params"]["s"]])


def _kmer_space(kw):
    return float(len(kw.get("alphabet", "ACGT"))) ** kw["k"] / (1.0 if kw.get("noncanonical") else 2.0)


def _hash_range(kw):
    return 2.0 ** 64 if float(len(kw.get("alphabet", "ACGT"))) ** kw["k"] > 2.0 ** 32 else 2.0 ** 32      # mg_params_init: use64


def _seed_threshold(case, recs):
    """the threshold seed_thresholds (host_sketch.cpp) starts the batch with, or None where its rule leaves the batch unseeded"""
    kw = case["params"]
    npos = helpers.screen_batch_npos(case, recs)
    if npos < 1:
        return None
    frac = 3.0 * kw["s"] / npos
    if frac >= 0.25 or _kmer_space(kw) < 64.0 * npos:
        return None
    return int(frac * _hash_range(kw))


def _holds_run(oracle, case, recs, kmer, run):
    """some record (some frame of it) holds `run` consecutive starts of `kmer`, a k-mer of one letter"""
    assert len(set(kmer)) == 1
    needle = kmer[:1] * (run + len(kmer) - 1)
    return any(needle in x for r in recs if len(r) >= len(needle) for x in (oracle.six_frames(r) if case["translate"] else [r]))


@pytest.mark.parametrize("name", helpers.SCREEN_CASES)
def test_screen_cases_meet_their_conditions(oracle, screen_cases, name):
    case, (table, nhash, lengths), counts, mix, rows = screen_cases[name]
    kw = case["params"]
    k, s = kw["k"], kw["s"]
    keys = set(table[i, j] for i in range(len(nhash)) for j in range(nhash[i]))
    distinct = [np.unique(helpers.screen_batch_hashes(oracle, kw, recs, case["translate"])) for recs in case["batches"]]

    # ---- every case: a database row that the mixture never touches, and (flood, short) counts that a double count would move far
    assert any(nhash[i] > 0 and not rows[i].any() for i in case["unsampled"])
    assert (rows > 0).sum() > 100 and len(mix) == s
    if case["hot"]:
        assert rows.max() >= case["hot"]

    if name.startswith("flood"):
        tile = TILE_SMALL if s <= S_SMALL_MAX else TILE_WIDE
        assert case["runs"]
        for b, kmer, run in case["runs"]:
            (h,) = helpers.screen_batch_hashes(oracle, kw, [kmer]).tolist()
            assert h in keys                                                    # the run's hash is a key of the database
            alone = distinct[b][:s]                                             # the sketch of the batch taken alone
            assert len(alone) == s and h in alone and h < alone[-1]             # every occurrence passes h < T, in every chunk
            assert run >= 3 * tile and _holds_run(oracle, case, case["batches"][b], kmer, run)
            assert counts[h] >= run
        for b, recs in enumerate(case["batches"]):
            # no batch comes out short of its seed: the flood cases reach the overflow path and leave the re-run alone
            t = _seed_threshold(case, recs)
            assert t is not None and (distinct[b] < t).sum() >= s, (b, t, int((distinct[b] < t).sum()))
        hot = [i for i in range(len(nhash)) if rows[i].max() >= case["hot"]]
        assert len(hot) >= 2                                                    # rows that share the flooded key: each gets its hit
        if name == "flood_forward":
            assert rows[0, 0] == rows[1, 0] != rows[2, 0] and table[0, 0] != table[2, 0]       # the T run is a key of its own
        elif not case["translate"]:
            assert table[0, 0] == table[1, 0] == table[2, 0] and rows[0, 0] == rows[1, 0] == rows[2, 0] >= sum(r for _, _, r in case["runs"])
        if name == "flood_wide":
            assert s > S_SMALL_MAX
    elif name == "short":
        assert sorted(case["short"]) == [0, 1]
        for b, kind in case["short"].items():
            t = _seed_threshold(case, case["batches"][b])
            assert t is not None                                                # 3 s / npos < 0.25 and kmer_space >= 64 npos
            if kind == "a":
                assert len(distinct[b]) < s                                     # fewer than s hashes at all
            else:
                assert len(distinct[b]) >= s and (distinct[b] < t).sum() < s    # enough hashes, too few below the seed
        small, mid = rows[7, : nhash[7]], rows[8, : nhash[8]]
        assert nhash[7] < s and set(small.tolist()) == {399, 400}               # (399: the k-mers across the unit's seam)
        assert set(mid.tolist()) <= {119, 120} and 120 in mid
    elif name == "batch_edges":
        sizes = [len(d) for d in distinct]
        assert sizes[0] == 0 and sizes[1] == 1 and distinct[1][0] in keys and sizes[2] == 0 and sizes[5] == 0 and sizes[6] == 1
        assert helpers.screen_batch_npos(case, case["batches"][0]) < 1 and helpers.screen_batch_npos(case, case["batches"][1]) == 1
        assert helpers.screen_batch_npos(case, case["batches"][2]) == 1
        first, second = (helpers.screen_blob(case["batches"][b]).tobytes() for b in (3, 4))
        assert sizes[3] > 1000 and first[:1] == first[-1:] == b"\n" and sizes[4] > 1000 and b"\n\n\n" in second
    else:
        raise AssertionError(name)
