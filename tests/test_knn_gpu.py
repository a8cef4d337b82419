"""`mash triangle -N` and mg_compare_tri_topk_host on the device.

Through the command: for every recorded case of tests/golden/knn (stdout of the REFERENCE CLI's `triangle -E`,
tests/golden/make_knn_golden.py) and N in {1, 3, 10}, the device route and the host route (MASH_AMD_HOST_FINISH=1) print exactly
what tests/knn_model.py makes of the recorded stdout, with equal stderr.
Through the C ABI: field for field and doubles bit for bit against the model over mg_compare_tri_pairs_host (the existing,
oracle-verified call), a sample against the oracle itself; every route (the mirrored candidate lists, the matrix with the
diagonal masked, forced engines, many blocks, many row chunks)."""
import ctypes as C
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

from mash_amd import abi
from tests import knn_model as km
from workloads import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASH = os.path.join(ROOT, "mash_amd", "bin", "mash")
GOLD = os.path.join(ROOT, "tests", "golden")
KSPACE21 = 4.0 ** 21
NS = (1, 3, 10)
TOPK_MAX = 1024
PAD = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope="module")
def eng():
    import torch
    torch.cuda.init()          # (torch ships its own HIP runtime: it initialises first, tests/test_gpu_parity.py)
    e = abi.MashGpu(0)
    e.set_option("MASHGPU_COSTS_FIXED", "1")
    yield e
    e.close()


# ------------------------------------------------------------------------------------------ through the command

def mash(args, cwd, host_route):
    env = dict(os.environ)
    env.pop("MASH_AMD_HOST_FINISH", None)
    if host_route:
        env["MASH_AMD_HOST_FINISH"] = "1"
    r = subprocess.run([MASH, *args], cwd=cwd, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def recorded():
    d = os.path.join(GOLD, "knn")
    cases = json.load(open(os.path.join(d, "cases.json")))
    return cases, os.path.join(GOLD, cases["input_dir"]), {c["name"]: open(os.path.join(d, c["name"] + ".out")).read() for c in cases["cases"]}


def test_command_on_the_recorded_family():
    cases, cwd, outs = recorded()
    for c in cases["cases"]:
        opts = [a for a in c["cmd"] if a != "-E"]                                # -N implies the edge list
        for n in NS:
            want = km.knn_of_stdout(outs[c["name"]], cases["names"], n)
            assert want
            dev = mash([*opts, "-N", str(n), *cases["inputs"]], cwd, False)
            host = mash([*opts, "-N", str(n), *cases["inputs"]], cwd, True)
            assert dev.stdout == want, (c["name"], n, "device route")
            assert host.stdout == want, (c["name"], n, "host route")
            assert dev.stderr == host.stderr
    # -E with it is redundant; N beyond the table is clamped: every other sketch, ranked
    want = km.knn_of_stdout(outs["triangle_d"], cases["names"], 3)
    assert mash(["triangle", "-i", "-k", "16", "-s", "64", "-E", "-d", "0.08", "-N", "3", *cases["inputs"]], cwd, False).stdout == want
    want = km.knn_of_stdout(outs["triangle"], cases["names"], 1000)
    assert len(want.splitlines()) == 43 * 42
    assert mash(["triangle", "-i", "-k", "16", "-s", "64", "-N", "1000", *cases["inputs"]], cwd, False).stdout == want


def test_command_composes_with_comment_threads_and_list(tmp_path):
    cases, cwd, outs = recorded()
    want = km.knn_of_stdout(outs["triangle"], cases["names"], 3)
    files = [os.path.join(cwd, f) for f in cases["inputs"]]
    lst = tmp_path / "in.txt"
    lst.write_text("".join(f + "\n" for f in files))
    assert mash(["triangle", "-i", "-k", "16", "-s", "64", "-p", "3", "-l", "-N", "3", str(lst)], str(tmp_path), False).stdout == want
    # -C prints the comments in place of the names (CommandTriangle.cpp:159-198): the same lines in the same order
    comment = {}
    for f in files:
        for ln in (gzip.open(f, "rt") if f.endswith(".gz") else open(f)):
            if ln.startswith(">"):
                name, _, rest = ln[1:].rstrip("\n").partition(" ")
                comment[name] = rest
    r = mash(["triangle", "-i", "-k", "16", "-s", "64", "-C", "-N", "3", *files], str(tmp_path), False)
    plain = [ln.split("\t") for ln in want.splitlines()]
    got = [ln.split("\t") for ln in r.stdout.splitlines()]
    assert len(got) == len(plain)
    for g, w in zip(got, plain):
        assert g[0] == comment[w[0]] and g[1] == comment[w[1]] and g[2:] == w[2:]


# ------------------------------------------------------------------------------------------ through the C ABI

def expected(pairs, n, k, ranked=None, row_begin=0, row_end=None):
    """the model over the packed triangle of mg_pair records -> RESULT_DTYPE records of rows [row_begin, row_end)"""
    order, count = ranked if ranked is not None else km.rank_rows(pairs["numer"], pairs["denom"], pairs["pass"], n)
    row_end = n if row_end is None else min(row_end, n)
    rows, cols = [], []
    for i in range(row_begin, row_end):
        c = np.asarray(order[i][:min(k, int(count[i]))], dtype=np.int64)
        cols.append(c)
        rows.append(np.full(len(c), i, dtype=np.int64))
    rows = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
    cols = np.concatenate(cols) if cols else np.zeros(0, dtype=np.int64)
    hi, lo = np.maximum(rows, cols), np.minimum(rows, cols)
    t = pairs[hi * (hi - 1) // 2 + lo]                                            # the record of the unordered pair
    out = np.zeros(len(rows), dtype=abi.RESULT_DTYPE)
    out["row"], out["col"] = rows, cols
    for f in ("numer", "denom", "distance", "p_value"):
        out[f] = t[f]
    return out


def same(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for f in ("row", "col", "numer", "denom"):
        assert np.array_equal(got[f], want[f]), f
    for f in ("distance", "p_value"):
        assert np.array_equal(got[f].view(np.uint64), want[f].view(np.uint64)), f      # bit for bit


def table_of(rows, s):
    t = np.full((len(rows), s), PAD, dtype=np.uint64)
    nh = np.zeros(len(rows), dtype=np.uint32)
    for i, r in enumerate(rows):
        r = np.unique(np.asarray(r, dtype=np.uint64))[:s]
        t[i, : len(r)] = r
        nh[i] = len(r)
    return t, nh


class options:
    def __init__(self, eng, opts):
        self.eng, self.opts = eng, opts

    def __enter__(self):
        for o, v in self.opts.items():
            self.eng.set_option(o, v)

    def __exit__(self, *exc):
        for o in self.opts:
            self.eng.set_option(o, None)


FILTERS = {"off": (-1.0, -1.0), "d": (0.05, -1.0), "v": (-1.0, 1e-10), "both": (0.05, 1e-10)}
# (with a filter on, many blocks need the matrix asked for: the default route has lists and no blocks; many row chunks go with the
# forced index engine, so that the chunks are chunks of the mirrored lists whatever the default engine makes of a job this small)
ROUTES = {"default": {}, "matrix": {"MASHGPU_RESULTS_MATRIX": "1"}, "sparse": {"MASHGPU_COMPARE_KERNEL": "sparse"},
          "blocks": {"MASHGPU_TOPK_BLOCK_PAIRS": str(3000 * 37), "MASHGPU_RESULTS_MATRIX": "1"}, "rows": {"MASHGPU_KNN_ROWS": "700", "MASHGPU_COMPARE_KERNEL": "sparse"}}
TABLES = {"clades": dict(n=3000, clusters=30, seed=3),          # clades of 100: degrees above 64 under -d 0.05
          "one_clade": dict(n=2500, clusters=1, seed=4)}         # every degree 2499, above the LDS buffer: 3.1e6 pairs


@pytest.fixture(scope="module", params=list(TABLES))
def big(eng, request):
    p = TABLES[request.param]
    table, nh, lengths = synth.clustered_sketches(p["n"], 1000, clusters=p["clusters"], seed=p["seed"])
    t = eng.table_upload(table, nh, lengths)
    yield {"name": request.param, "t": t, "n": p["n"], "table": table, "nh": nh, "lengths": lengths}
    t.free()


@pytest.mark.parametrize("filt", list(FILTERS))
def test_big_table_every_k_every_route(eng, oracle, big, filt):
    max_d, max_p = FILTERS[filt]
    n = big["n"]
    pairs = eng.compare_tri_pairs(big["t"], 21, KSPACE21, max_d, max_p)
    ranked = km.rank_rows(pairs["numer"], pairs["denom"], pairs["pass"], n)
    if big["name"] == "one_clade":
        assert np.all(ranked[1] == n - 1)                          # every pair passes every filter: all degrees 2499
    elif filt != "off":
        assert 64 < ranked[1].max() < n - 1 and 0 < ranked[1].sum()               # the filter bites, and something is left
    sample = []
    for k in (1, 10, 100, TOPK_MAX):
        want = expected(pairs, n, k, ranked)
        assert len(want)
        for route, opts in ROUTES.items():
            with options(eng, opts):
                got = eng.compare_tri_topk(big["t"], 21, KSPACE21, k, max_d, max_p)
            same(got, want)
        if k == 100:
            sample = want
    # a sample of 2000 of the returned records against the oracle itself: the record of the unordered pair, the later row the query
    rng = np.random.default_rng(11)
    for e in sample[rng.choice(len(sample), 2000, replace=False)]:
        hi, lo = max(int(e["row"]), int(e["col"])), min(int(e["row"]), int(e["col"]))
        o = oracle.compare(big["table"][lo, : big["nh"][lo]], big["table"][hi, : big["nh"][hi]], int(big["lengths"][lo]), int(big["lengths"][hi]),
                           1000, 21, KSPACE21, max_d, max_p)
        assert o.pass_ and (o.numer, o.denom) == (int(e["numer"]), int(e["denom"]))
        assert o.distance == e["distance"] and o.p_value == e["p_value"]


def test_resident_table_changing_k_and_ranges(eng, big):
    n = big["n"]
    for max_d in (-1.0, 0.05):
        pairs = eng.compare_tri_pairs(big["t"], 21, KSPACE21, max_d, -1.0)
        ranked = km.rank_rows(pairs["numer"], pairs["denom"], pairs["pass"], n)
        for k, rb, re in ((5, 100, 130), (1, 0, 7), (50, n - 3, n + 50), (5, 100, 130), (TOPK_MAX, 1234, 1236)):
            same(eng.compare_tri_topk(big["t"], 21, KSPACE21, k, max_d, row_begin=rb, row_end=re), expected(pairs, n, k, ranked, rb, re))
        assert len(eng.compare_tri_topk(big["t"], 21, KSPACE21, 3, max_d, row_begin=40, row_end=40)) == 0      # an empty range
        assert len(eng.compare_tri_topk(big["t"], 21, KSPACE21, 3, max_d, row_begin=n, row_end=n + 100)) == 0  # beyond the table


def test_symmetry_and_the_p_value_boundary_on_both_routes(eng):
    """Sketches of 16 hashes over a universe of 150 values, lengths from 500 to 50 000, k = 8: pairs share 0 .. 6 hashes and their
    p-values spread over many orders of magnitude around the threshold, with a different length on either side of every pair.
    k >= the largest degree, so a pair is in both its rows' lists or in neither -- and the matrix route, which evaluates the p-value
    with the two lengths in (row, neighbour) order, agrees with the list route, which evaluates it once in the triangle's order."""
    rng = np.random.default_rng(21)
    n, s, kspace = 400, 16, 4.0 ** 8
    t, nh = table_of([rng.choice(150, int(rng.integers(3, 17)), replace=False) + 1 for _ in range(n)], s)
    lengths = rng.integers(500, 50_000, n).astype(np.uint64)
    tab = eng.table_upload(t, nh, lengths)
    for max_d, max_p in ((-1.0, 1e-3), (0.2, 1e-2), (0.15, -1.0)):
        pairs = eng.compare_tri_pairs(tab, 8, kspace, max_d, max_p)
        assert 0 < pairs["pass"].sum() < len(pairs)
        want = expected(pairs, n, n - 1)
        got = eng.compare_tri_topk(tab, 8, kspace, n - 1, max_d, max_p)
        with options(eng, {"MASHGPU_RESULTS_MATRIX": "1"}):
            got_m = eng.compare_tri_topk(tab, 8, kspace, n - 1, max_d, max_p)
        same(got, want)
        same(got_m, want)
        assert len(got) == 2 * int(pairs["pass"].sum())
        back = {(int(e["row"]), int(e["col"])): e for e in got}
        for e in got:
            m = back[(int(e["col"]), int(e["row"]))]
            assert (m["numer"], m["denom"]) == (e["numer"], e["denom"])
            assert m["distance"].tobytes() == e["distance"].tobytes() and m["p_value"].tobytes() == e["p_value"].tobytes()
    tab.free()


SMALL_ROUTES = {"default": {}, "matrix": {"MASHGPU_RESULTS_MATRIX": "1"}, "sparse": {"MASHGPU_COMPARE_KERNEL": "sparse"},
                "blocks": {"MASHGPU_TOPK_BLOCK_PAIRS": "9", "MASHGPU_RESULTS_MATRIX": "1"}, "rows": {"MASHGPU_KNN_ROWS": "3", "MASHGPU_COMPARE_KERNEL": "sparse"}}


def test_small_tables_zero_numerators_ties_and_clamps(eng):
    S = 8
    base = np.arange(1, 9, dtype=np.uint64) * np.uint64(100)
    far = lambda i: np.arange(1, 9, dtype=np.uint64) * np.uint64(100) + np.uint64(10_000 * (i + 1))
    one = lambda rows: eng.table_upload(*table_of(rows, S), np.full(len(rows), 50_000, dtype=np.uint64))
    # n = 1: nobody has a neighbour; n = 2: each other's
    t = one([base])
    assert len(eng.compare_tri_topk(t, 21, KSPACE21, 3)) == 0 and len(eng.compare_tri_topk(t, 21, KSPACE21, 3, max_d=0.1)) == 0
    t.free()
    t = one([base, base])
    for max_d in (-1.0, 0.1):
        got = eng.compare_tri_topk(t, 21, KSPACE21, 5, max_d)
        assert [(int(e["row"]), int(e["col"]), int(e["numer"])) for e in got] == [(0, 1, 8), (1, 0, 8)]
    t.free()
    # row 7 shares nothing with anybody.  Row 4: row 2 holds its LARGEST hash only, behind the first s union elements (an index
    # candidate with numer 0 among non-candidates), row 5 shares four hashes, row 8 is its copy, row 6 is ragged (3 hashes)
    q1 = base + np.uint64(5)
    r2 = np.concatenate([np.arange(1, 8, dtype=np.uint64), q1[-1:]])
    r5 = np.concatenate([q1[:4], far(7)[:4]])
    t = one([far(0), far(1), r2, far(3), q1, r5, far(6)[:3], far(20), q1])
    pairs = eng.compare_tri_pairs(t, 21, KSPACE21)
    assert int(pairs[km.tri_index(4, 2)]["numer"]) == 0 and int(pairs[km.tri_index(5, 4)]["numer"]) == 4 and int(pairs[km.tri_index(8, 4)]["numer"]) == 8
    pd = eng.compare_tri_pairs(t, 21, KSPACE21, 0.3, -1.0)
    for opts in SMALL_ROUTES.values():
        with options(eng, opts):
            for k in (1, 3, 5, 8, 100):                                                  # (k > n - 1 is clamped)
                got = eng.compare_tri_topk(t, 21, KSPACE21, k)
                same(got, expected(pairs, 9, k))
                kk = min(k, 8)
                r7 = got[got["row"] == 7]
                assert list(r7["col"]) == [0, 1, 2, 3, 4, 5, 6, 8][:kk]                  # nothing shared: index order, across the diagonal,
                assert np.all(r7["distance"] == 1.0) and np.all(r7["p_value"] == 1.0)    # distance 1, p-value 1
                r4 = got[got["row"] == 4]
                assert list(r4["col"]) == [8, 5, 0, 1, 2, 3, 6, 7][:kk]                  # ... the 0-numer candidate (2) not before 0 and 1
            got = eng.compare_tri_topk(t, 21, KSPACE21, 5, max_d=0.3)
            same(got, expected(pd, 9, 5))
            assert sorted(set(got["row"].tolist())) == [4, 5, 8]                         # no record for a row that shares nothing
    t.free()
    # two empty sketches (0/0) among others
    t = one([base, [], [], far(1), base[:5]])
    for max_d in (-1.0, 0.4):
        pairs = eng.compare_tri_pairs(t, 21, KSPACE21, max_d, -1.0)
        assert (int(pairs[km.tri_index(2, 1)]["numer"]), int(pairs[km.tri_index(2, 1)]["denom"])) == (0, 0)
        for opts in SMALL_ROUTES.values():
            with options(eng, opts):
                for k in (1, 2, 4):
                    same(eng.compare_tri_topk(t, 21, KSPACE21, k, max_d), expected(pairs, 5, k))
    t.free()
    # identical rows: a full tie, cut in index order with the row itself skipped
    t = one([base] * 50)
    for k in (1, 7, 49, 64):
        for max_d in (-1.0, 0.1):
            got = eng.compare_tri_topk(t, 21, KSPACE21, k, max_d)
            kk = min(k, 49)
            assert len(got) == 50 * kk and np.all(got["numer"] == 8)
            for i in (0, 1, 24, 48, 49):
                assert list(got["col"][i * kk:(i + 1) * kk]) == [j for j in range(50) if j != i][:kk]
    t.free()


def test_capacity_and_error_paths(eng):
    lib = eng.lib
    table, nh, lengths = synth.clustered_sketches(300, 1000, clusters=3, seed=9)
    tab = eng.table_upload(table, nh, lengths)
    n = C.c_uint64(0)

    def call(t, k, out, cap, cnt, r0=0, r1=8):
        return lib.mg_compare_tri_topk_host(eng.ctx, t, r0, r1, 21, KSPACE21, -1.0, -1.0, k, out, cap, cnt)

    buf = np.zeros(80, dtype=abi.RESULT_DTYPE)
    assert call(tab.handle, 10, buf.ctypes.data, 79, C.byref(n)) == abi.MG_ERR_NOMEM and n.value == 80
    assert call(tab.handle, 10, None, 0, C.byref(n)) == abi.MG_ERR_NOMEM and n.value == 80
    assert call(tab.handle, 10, buf.ctypes.data, 80, C.byref(n)) == abi.MG_OK and n.value == 80
    same(buf, eng.compare_tri_topk(tab, 21, KSPACE21, 10, row_begin=0, row_end=8))
    assert call(tab.handle, 0, buf.ctypes.data, 80, C.byref(n)) == -1                              # MG_ERR_INVALID
    assert call(tab.handle, TOPK_MAX + 1, buf.ctypes.data, 80, C.byref(n)) == -2                    # MG_ERR_UNSUPPORTED
    assert call(None, 3, buf.ctypes.data, 80, C.byref(n)) == -1
    assert call(tab.handle, 3, None, 80, C.byref(n)) == -1
    assert call(tab.handle, 3, buf.ctypes.data, 80, None) == -1
    bare = eng.table_upload(table[:4], nh[:4])                                                      # a table without lengths
    assert call(bare.handle, 3, buf.ctypes.data, 80, C.byref(n)) == -1
    bare.free()
    # the list route: the count of a thresholded call, too small a buffer, then the right one
    want = eng.compare_tri_topk(tab, 21, KSPACE21, 10, max_d=0.05, row_begin=0, row_end=8)
    rc = lib.mg_compare_tri_topk_host(eng.ctx, tab.handle, 0, 8, 21, KSPACE21, 0.05, -1.0, 10, buf.ctypes.data, 5, C.byref(n))
    assert rc == abi.MG_ERR_NOMEM and n.value == len(want) == 80
    assert call(tab.handle, 2, buf.ctypes.data, 80, C.byref(n)) == abi.MG_OK and n.value == 16      # the context still works
    tab.free()
