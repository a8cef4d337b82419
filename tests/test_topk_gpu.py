"""`mash dist -N` and mg_compare_rect_topk_host on the device.

Through the command: for every recorded case of tests/golden/topk (stdout of the REFERENCE CLI, tests/golden/make_topk_golden.py)
and N in {1, 3, 10}, the device route and the host route (MASH_AMD_HOST_FINISH=1) print exactly what tests/topk_model.py makes
of the recorded stdout, with equal stderr; the same on the dist_individual / x_dist_protein inputs of tests/golden/cli.
Through the C ABI: field for field and doubles bit for bit against the model over mg_compare_rect_pairs_host (the existing,
oracle-verified call), a sample against the oracle itself."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from mash_amd import abi
from tests import topk_model as tm
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


def check_command(cmd, inputs, cwd, recorded, ns=NS):
    for n in ns:
        want = tm.topk_of_stdout(recorded, n)
        dev = mash([*cmd, "-N", str(n), *inputs], cwd, False)
        host = mash([*cmd, "-N", str(n), *inputs], cwd, True)
        assert dev.stdout == want, (cmd, n, "device route")
        assert host.stdout == want, (cmd, n, "host route")
        assert dev.stderr == host.stderr


def test_recorded_fixture_meets_its_conditions():
    d = os.path.join(GOLD, "topk")
    cases = json.load(open(os.path.join(d, "cases.json")))
    plain = open(os.path.join(d, "dist.out")).read()
    for n in NS:
        assert tm.has_tie_across_cut(plain, n), n
    lines = [len(l) for _, l in tm.query_runs(open(os.path.join(d, "dist_d.out")).read())]
    assert any(0 < x < 3 for x in lines) and any(0 < x < 10 for x in lines) and any(x >= 10 for x in lines)
    assert len(lines) < cases["queries"]                          # a query without a line under -d
    assert len(tm.query_runs(plain)) == cases["queries"]


def test_command_on_the_recorded_family():
    d = os.path.join(GOLD, "topk")
    cases = json.load(open(os.path.join(d, "cases.json")))
    for c in cases["cases"]:
        check_command(c["cmd"], cases["inputs"], d, open(os.path.join(d, c["name"] + ".out")).read())


def test_command_composes_with_comment_threads_list_and_sketch_files(tmp_path):
    d = os.path.join(GOLD, "topk")
    recorded = open(os.path.join(d, "dist.out")).read()
    fam, out = os.path.join(d, "family.fa.gz"), os.path.join(d, "outsiders.fa")
    want = tm.topk_of_stdout(recorded, 3)
    lst = tmp_path / "q.txt"
    lst.write_text(fam + "\n" + out + "\n")
    r = mash(["dist", "-i", "-k", "16", "-s", "64", "-p", "3", "-l", "-N", "3", fam, str(lst)], str(tmp_path), False)
    assert r.stdout == want
    mash(["sketch", "-i", "-k", "16", "-s", "64", "-o", "fam", fam], str(tmp_path), False)
    r = mash(["dist", "-i", "-N", "3", "fam.msh", fam, out], str(tmp_path), False)
    assert r.stdout == want
    # -C appends the comments to both names: the same lines in the same order
    r = mash(["dist", "-i", "-k", "16", "-s", "64", "-C", "-N", "3", fam, fam, out], str(tmp_path), False)
    plain = [ln.split("\t") for ln in want.splitlines()]
    got = [ln.split("\t") for ln in r.stdout.splitlines()]
    assert len(got) == len(plain)
    for g, w in zip(got, plain):
        assert g[0].split(":")[0] == w[0] and g[1].split(":")[0] == w[1] and g[2:] == w[2:]


@pytest.mark.parametrize("name", ["dist_individual", "x_dist_protein"])
def test_command_on_the_cli_goldens(name):
    d = os.path.join(GOLD, "cli")
    case = [c for c in json.load(open(os.path.join(d, "cases.json"))) if c["name"] == name][0]
    assert not case["setup"]
    opts = [a for a in case["cmd"] if not a.endswith(".fa")]
    inputs = [a for a in case["cmd"] if a.endswith(".fa")]
    check_command(opts, inputs, os.path.join(d, "in"), open(os.path.join(d, name + ".out")).read(), ns=(1, 2, 3, 10))


# ------------------------------------------------------------------------------------------ through the C ABI

def expected(pairs, k, q_begin=0):
    """the model over a matrix of mg_pair records -> RESULT_DTYPE records"""
    out = []
    for q in range(pairs.shape[0]):
        row = pairs[q]
        for r in tm.rank_row_fast(row["numer"], row["denom"], row["pass"], k):
            out.append((q_begin + q, r, row["numer"][r], row["denom"][r], row["distance"][r], row["p_value"][r]))
    return np.array(out, dtype=abi.RESULT_DTYPE) if out else np.zeros(0, dtype=abi.RESULT_DTYPE)


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


FILTERS = {"off": (-1.0, -1.0), "d": (0.05, -1.0), "v": (-1.0, 1e-10), "both": (0.05, 1e-10)}
ROUTES = {"default": {}, "matrix": {"MASHGPU_RESULTS_MATRIX": "1"}, "sparse": {"MASHGPU_COMPARE_KERNEL": "sparse"},
          "blocks": {"MASHGPU_TOPK_BLOCK_PAIRS": str(20000 * 37)}}


@pytest.fixture(scope="module")
def big(eng):
    """20 000 clustered references x 512 queries: 256 drawn from the clades, 128 random, 128 copies of references"""
    NREF, S = 20000, 1000
    table, nh, lengths = synth.clustered_sketches(NREF, S, seed=3)
    qt, qn, _ = synth.clustered_sketches(256, S, clusters=NREF // 100, seed=77)
    rng = np.random.default_rng(5)
    rnd = np.sort(rng.integers(0, 1 << 54, (128, S), dtype=np.uint64), axis=1)
    cp = rng.choice(NREF, 128, replace=False)
    qtab = np.concatenate([qt, rnd, table[cp]], 0)
    qnh = np.concatenate([qn, np.full(128, S, dtype=np.uint32), nh[cp]])
    qlen = np.full(512, 1_200_000, dtype=np.uint64)
    ref, qry = eng.table_upload(table, nh, lengths), eng.table_upload(qtab, qnh, qlen)
    yield {"ref": ref, "qry": qry, "table": table, "nh": nh, "lengths": lengths, "qtab": qtab, "qnh": qnh, "qlen": qlen}
    ref.free()
    qry.free()


@pytest.mark.parametrize("filt", list(FILTERS))
def test_big_table_every_k_every_route(eng, oracle, big, filt):
    max_d, max_p = FILTERS[filt]
    pairs = eng.compare_rect_pairs(big["ref"], big["qry"], 21, KSPACE21, max_d, max_p)
    sample = []
    for k in (1, 10, 100, TOPK_MAX):
        want = expected(pairs, k)
        if filt != "off":
            assert 0 < len(want) < 512 * k                         # the filter bites, and something is left
        for route, opts in ROUTES.items():
            for o, v in opts.items():
                eng.set_option(o, v)
            try:
                got = eng.compare_rect_topk(big["ref"], big["qry"], 21, KSPACE21, k, max_d, max_p)
            finally:
                for o in opts:
                    eng.set_option(o, None)
            same(got, want)
        if k == 100:
            sample = want
    # a sample of 2000 of the returned records (all of them where a filter leaves fewer) against the oracle itself
    rng = np.random.default_rng(11)
    pick = rng.choice(len(sample), min(len(sample), 2000), replace=False)
    assert len(pick) == 2000 or filt != "off"
    for e in sample[pick]:
        q, r = int(e["row"]), int(e["col"])
        o = oracle.compare(big["table"][r, : big["nh"][r]], big["qtab"][q, : big["qnh"][q]], int(big["lengths"][r]), int(big["qlen"][q]),
                           1000, 21, KSPACE21, max_d, max_p)
        assert o.pass_ and (o.numer, o.denom) == (int(e["numer"]), int(e["denom"]))
        assert o.distance == e["distance"] and o.p_value == e["p_value"]


def test_resident_table_changing_k_and_ranges(eng, big):
    pairs = eng.compare_rect_pairs(big["ref"], big["qry"], 21, KSPACE21, -1.0, -1.0, 250, 262)
    for k in (5, 1, 50, 5, 20001):
        same(eng.compare_rect_topk(big["ref"], big["qry"], 21, KSPACE21, min(k, TOPK_MAX), q_begin=250, q_end=262), expected(pairs, min(k, TOPK_MAX), 250))
    assert len(eng.compare_rect_topk(big["ref"], big["qry"], 21, KSPACE21, 3, q_begin=40, q_end=40)) == 0       # an empty range
    assert len(eng.compare_rect_topk(big["ref"], big["qry"], 21, KSPACE21, 3, q_begin=600, q_end=700)) == 0


@pytest.mark.parametrize("scale", [1, 10])
def test_near_equal_fractions(eng, scale):
    """4999/9999 < 5000/10001 < 5000/10000 (and tenfold), stored worst first: index order is the wrong answer, and so is any
    float32 key"""
    s = 10002 if scale == 1 else 100002
    nq, sizes, shared = 7500 * scale, (7500 * scale - 2, 7500 * scale + 1, 7500 * scale), (5000 * scale - 1, 5000 * scale, 5000 * scale)
    q = np.arange(1, nq + 1, dtype=np.uint64) * np.uint64(1000)
    rows = []
    for i, (n, c) in enumerate(zip(sizes, shared)):
        own = np.arange(1, n - c + 1, dtype=np.uint64) * np.uint64(1000) + np.uint64(i + 1)
        rows.append(np.concatenate([q[np.arange(c) * nq // c], own]))
    rt, rn = table_of(rows, s)
    qt, qn = table_of([q], s)
    assert list(rn) == list(sizes) and qn[0] == nq
    ref = eng.table_upload(rt, rn, np.full(3, 3_000_000, dtype=np.uint64))
    qry = eng.table_upload(qt, qn, np.full(1, 3_000_000, dtype=np.uint64))
    pairs = eng.compare_rect_pairs(ref, qry, 21, KSPACE21)
    w = 1 if scale == 1 else 10
    assert [(int(p["numer"]), int(p["denom"])) for p in pairs[0]] == [(5000 * w - 1, 10000 * w - 1), (5000 * w, 10000 * w + 1), (5000 * w, 10000 * w)]
    for k, cols in ((2, [2, 1]), (3, [2, 1, 0])):
        for opts in ROUTES.values():
            for o, v in opts.items():
                eng.set_option(o, "3" if o == "MASHGPU_TOPK_BLOCK_PAIRS" else v)
            try:
                got = eng.compare_rect_topk(ref, qry, 21, KSPACE21, k)
                got_d = eng.compare_rect_topk(ref, qry, 21, KSPACE21, k, max_d=0.5)
            finally:
                for o in opts:
                    eng.set_option(o, None)
            assert list(got["col"]) == cols
            same(got, expected(pairs, k))
            same(got_d, expected(pairs, k))
    ref.free()
    qry.free()


def test_small_tables_zero_numerators_ties_and_clamps(eng):
    S = 8
    base = np.arange(1, 9, dtype=np.uint64) * np.uint64(100)
    far = lambda i: np.arange(1, 9, dtype=np.uint64) * np.uint64(100) + np.uint64(10_000 * (i + 1))
    # query 0 shares nothing with anybody; query 1: reference 2 holds its LARGEST hash only, behind the first s union elements
    # (an index candidate with numer 0 among non-candidates), reference 4 is its copy, reference 5 shares four hashes
    q1 = base + np.uint64(5)
    r2 = np.concatenate([np.arange(1, 8, dtype=np.uint64), q1[-1:]])
    r5 = np.concatenate([q1[:4], far(7)[:4]])
    rt, rn = table_of([far(0), far(1), r2, far(3), q1, r5, far(6)[:3]], S)                # (ragged: the last row holds 3 hashes)
    qt, qn = table_of([far(20), q1], S)
    ref = eng.table_upload(rt, rn, np.full(7, 50_000, dtype=np.uint64))
    qry = eng.table_upload(qt, qn, np.full(2, 60_000, dtype=np.uint64))
    pairs = eng.compare_rect_pairs(ref, qry, 21, KSPACE21)
    assert int(pairs[1, 2]["numer"]) == 0 and int(pairs[1, 4]["numer"]) == 8 and int(pairs[1, 5]["numer"]) == 4
    for opts in ROUTES.values():
        for o, v in opts.items():
            eng.set_option(o, "7" if o == "MASHGPU_TOPK_BLOCK_PAIRS" else v)
        try:
            for k in (1, 3, 5, 7, 100):                                                  # (k > nref is clamped)
                got = eng.compare_rect_topk(ref, qry, 21, KSPACE21, k)
                same(got, expected(pairs, k))
                kk = min(k, 7)
                assert list(got["col"][:kk]) == list(range(kk))                          # nothing shared: index order,
                assert np.all(got["distance"][:kk] == 1.0) and np.all(got["p_value"][:kk] == 1.0)   # distance 1, p-value 1
                if k >= 3:
                    assert list(got["col"][kk:kk + 3]) == [4, 5, 0]                      # ... the 0-numer candidate (2) not before 0 and 1
            pd = eng.compare_rect_pairs(ref, qry, 21, KSPACE21, 0.3, -1.0)
            got = eng.compare_rect_topk(ref, qry, 21, KSPACE21, 5, max_d=0.3)
            same(got, expected(pd, 5))
            assert len(got) and not np.any(got["row"] == 0)                              # no row for the query that shares nothing
        finally:
            for o in opts:
                eng.set_option(o, None)
    ref.free()
    qry.free()
    # identical references: a full tie, cut in index order
    rt, rn = table_of([base] * 50, S)
    ref = eng.table_upload(rt, rn, np.full(50, 50_000, dtype=np.uint64))
    qt, qn = table_of([base, far(1)], S)
    qry = eng.table_upload(qt, qn, np.full(2, 60_000, dtype=np.uint64))
    for k in (1, 7, 50, 64):
        for filt in (-1.0, 0.1):
            got = eng.compare_rect_topk(ref, qry, 21, KSPACE21, k, max_d=filt)
            kk = min(k, 50)
            assert list(got["col"][:kk]) == list(range(kk)) and np.all(got["numer"][:kk] == 8)
            assert len(got) == (2 * kk if filt < 0 else kk)
    ref.free()
    qry.free()


def test_tables_of_different_sketch_size_and_ragged_rows(eng):
    t, nh, lengths = synth.clustered_sketches(300, 1000, clusters=3, seed=9)
    rng = np.random.default_rng(2)
    nh = nh.copy()
    for i in range(0, 300, 7):                                                            # ragged rows
        nh[i] = int(rng.integers(0, 900))
        t[i, nh[i]:] = PAD
    ref = eng.table_upload(t, nh, lengths)
    qry = eng.table_upload(np.ascontiguousarray(t[:40, :500]), np.minimum(nh[:40], 500).astype(np.uint32), lengths[:40])
    for max_d in (-1.0, 0.1):
        pairs = eng.compare_rect_pairs(ref, qry, 21, KSPACE21, max_d, -1.0)
        for k in (1, 10, 300):
            same(eng.compare_rect_topk(ref, qry, 21, KSPACE21, k, max_d=max_d), expected(pairs, k))
    ref.free()
    qry.free()


def test_capacity_and_error_paths(eng, big):
    lib = eng.lib
    ref, qry = big["ref"], big["qry"]
    n = C.c_uint64(0)

    def call(r, q, k, out, cap, cnt, q0=0, q1=8):
        return lib.mg_compare_rect_topk_host(eng.ctx, r, q, q0, q1, 21, KSPACE21, -1.0, -1.0, k, out, cap, cnt)

    buf = np.zeros(80, dtype=abi.RESULT_DTYPE)
    assert call(ref.handle, qry.handle, 10, buf.ctypes.data, 79, C.byref(n)) == abi.MG_ERR_NOMEM and n.value == 80
    assert call(ref.handle, qry.handle, 10, None, 0, C.byref(n)) == abi.MG_ERR_NOMEM and n.value == 80
    assert call(ref.handle, qry.handle, 10, buf.ctypes.data, 80, C.byref(n)) == abi.MG_OK and n.value == 80
    same(buf, eng.compare_rect_topk(ref, qry, 21, KSPACE21, 10, q_begin=0, q_end=8))
    assert call(ref.handle, qry.handle, 0, buf.ctypes.data, 80, C.byref(n)) == -1                  # MG_ERR_INVALID
    assert call(ref.handle, qry.handle, TOPK_MAX + 1, buf.ctypes.data, 80, C.byref(n)) == -2        # MG_ERR_UNSUPPORTED
    assert call(None, qry.handle, 3, buf.ctypes.data, 80, C.byref(n)) == -1
    assert call(ref.handle, None, 3, buf.ctypes.data, 80, C.byref(n)) == -1
    assert call(ref.handle, qry.handle, 3, None, 80, C.byref(n)) == -1
    assert call(ref.handle, qry.handle, 3, buf.ctypes.data, 80, None) == -1
    bare = eng.table_upload(big["qtab"][:4], big["qnh"][:4])                                        # a table without lengths
    assert call(ref.handle, bare.handle, 3, buf.ctypes.data, 80, C.byref(n)) == -1
    assert call(bare.handle, qry.handle, 3, buf.ctypes.data, 80, C.byref(n)) == -1
    bare.free()
    assert call(ref.handle, qry.handle, 2, buf.ctypes.data, 80, C.byref(n)) == abi.MG_OK and n.value == 16   # the context still works


def test_sharded_calls_equal_the_single_device_call(eng, big):
    comm = abi.LocalComm([0, 0, 0])
    table, nh, lengths = big["table"][:3001], big["nh"][:3001], big["lengths"][:3001]
    qtab, qnh, qlen = big["qtab"][200:300], big["qnh"][200:300], big["qlen"][200:300]
    ref, qry = eng.table_upload(table, nh, lengths), eng.table_upload(qtab, qnh, qlen)
    dq = comm.upload(qtab, qnh, qlen)
    for mode in ("replicated", "rows"):
        dr = comm.upload(table, nh, lengths) if mode == "replicated" else comm.upload_rows(table, nh, lengths)
        for max_d in (-1.0, 0.05):
            for k in (1, 10, TOPK_MAX):
                want = eng.compare_rect_topk(ref, qry, 21, KSPACE21, k, max_d=max_d)
                same(comm.compare_rect_topk(dr, dq, 21, KSPACE21, k, max_d=max_d, capacity=16), want)
        want = eng.compare_rect_topk(ref, qry, 21, KSPACE21, 4, q_begin=10, q_end=33)
        same(comm.compare_rect_topk(dr, dq, 21, KSPACE21, 4, q_begin=10, q_end=33), want)
        comm.free(dr)
    comm.free(dq)
    comm.close()
    ref.free()
    qry.free()
