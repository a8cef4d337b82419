"""`mash within`, mg_within_rect_host and mg_within_rect_results_host on the device, against tests/within_model.py.

Through the C ABI: {common, j} of every pair and the thresholded, compacted survivors on tables of 1 to 70 rows with sketch
sizes 1, 5, 64, 65 and 1000 -- and 5000: within.hip stages no row in LDS, so no sketch size takes another path; 5000 is the
largest tested --, tables of different sketch sizes either way round, rows of 0, 1 and fewer than s hashes (and a real hash equal
to the padding value), values below 2^32, one reference, one query, sub-ranges of the queries (empty and clamped ones too), several
device blocks per call, max_error on both sides of a j_min boundary and <= 0, >= 1, +inf and NaN, and the capacity protocol.
Through the command: every recorded case of tests/golden/within (stdout and exit status of the REFERENCE CLI), by the device
route and by the host route (MASH_AMD_HOST_FINISH=1), also cut into blocks of a few pairs."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from mash_amd import abi
from tests import within_fixture as wf
from tests import within_model as wm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASH = os.path.join(ROOT, "mash_amd", "bin", "mash")
PAD = 0xFFFFFFFFFFFFFFFF
MG_ERR_INVALID = -1


@pytest.fixture(scope="module")
def eng():
    import torch
    torch.cuda.init()          # (torch ships its own HIP runtime: it initialises first, tests/test_gpu_parity.py)
    e = abi.MashGpu(0)
    yield e
    e.close()


# ------------------------------------------------------------------------------------------ tables and their expectation

def make_table(rng, n, s, universe, ragged, limit=None):
    """n rows of up to s ascending distinct hashes out of one sorted pool of `universe` values (the same pool for every table of
    a seed-independent `universe`, so that rows of two tables share hashes); a row is a window of the pool -- low, high or
    wide -- so that a reference ends below, above or inside a query.  ragged: 0 full rows, 1 any count, 2 also 0 and 1."""
    pool = np.random.default_rng(universe).integers(0, limit or 2 ** 64, universe, dtype=np.uint64)
    pool = np.unique(pool)
    table = np.full((n, s), PAD, dtype=np.uint64)
    nhash = np.zeros(n, dtype=np.uint32)
    for r in range(n):
        want = s
        if ragged:
            want = int(rng.integers(0, s + 1))
        if ragged == 2 and r % 3 < 2:
            want = r % 3
        lo = int(rng.integers(0, len(pool)))
        span = int(rng.integers(1, len(pool) + 1))
        pick = np.unique(pool[(lo + rng.integers(0, span, want * 2)) % len(pool)])[:want]
        table[r, : len(pick)] = pick
        nhash[r] = len(pick)
    return table, nhash


def expected(ref, qry):
    """{common, j} of every pair, query-major, by the closed form in numpy (checked against the model's walk below)"""
    (rt, rn), (qt, qn) = ref, qry
    out = np.zeros((len(qn), len(rn)), dtype=abi.COUNTS_DTYPE)
    for q in range(len(qn)):
        Q = qt[q, : qn[q]]
        for r in range(len(rn)):
            R = rt[r, : rn[r]]
            if not len(R) or not len(Q):
                continue
            j = min(len(R), len(Q), int(np.searchsorted(Q, R[-1], side="right")))
            out[q, r] = (len(np.intersect1d(Q[:j], R, assume_unique=True)), j)
    return out


def survivors(exp, max_error, q_begin=0):
    thr = max_error
    rows = [(q_begin + q, r, exp[q, r]["numer"], exp[q, r]["denom"]) for q in range(exp.shape[0]) for r in range(exp.shape[1])
            if wm.passes(int(exp[q, r]["denom"]), thr)]
    return np.array(rows, dtype=abi.EDGE_DTYPE) if rows else np.zeros(0, dtype=abi.EDGE_DTYPE)


def upload(eng, t):
    return eng.table_upload(t[0], t[1])


def check_job(eng, ref, qry, errors=(1.0, 0.3, 0.13)):
    exp = expected(ref, qry)
    tr, tq = upload(eng, ref), upload(eng, qry)
    try:
        got = eng.within_rect_host(tr, tq)
        assert got.shape == exp.shape and np.array_equal(got, exp), np.argwhere(got != exp)[:5]
        for e in errors:
            res = eng.within_rect_results(tr, tq, e)
            want = survivors(exp, e)
            assert np.array_equal(res, want), (e, len(res), len(want))
            key = res["row"].astype(np.uint64) * np.uint64(len(ref[1])) + res["col"]
            assert np.all(np.diff(key.astype(np.int64)) > 0)                 # strictly ascending by (row, col)
    finally:
        tr.free()
        tq.free()
    return exp


def test_numpy_expectation_is_the_models_walk():
    rng = np.random.default_rng(1)
    ref, qry = make_table(rng, 9, 40, 90, 2), make_table(rng, 11, 25, 90, 2)
    exp = expected(ref, qry)
    seen = set()
    for q in range(11):
        for r in range(9):
            R, Q = [int(x) for x in ref[0][r, : ref[1][r]]], [int(x) for x in qry[0][q, : qry[1][q]]]
            assert tuple(exp[q, r]) == wm.walk(R, Q) == wm.closed(R, Q)
            seen.add(wm.termination(R, Q))
    assert seen == {"Q", "R", "exhausted", "empty"}


# ------------------------------------------------------------------------------------------ through the C ABI

@pytest.mark.parametrize("s,nref,nqry", [(1, 70, 33), (5, 70, 33), (64, 70, 33), (65, 33, 70), (64, 7, 9), (1000, 7, 9), (5000, 3, 4)])
@pytest.mark.parametrize("ragged", [0, 1])
def test_sketch_sizes_and_rows(eng, s, nref, nqry, ragged):
    rng = np.random.default_rng(s * 10 + ragged)
    exp = check_job(eng, make_table(rng, nref, s, 3 * s + 2, ragged), make_table(rng, nqry, s, 3 * s + 2, ragged))
    if s >= 64:
        assert (exp["numer"] > 0).any() and (exp["denom"] < s).any()          # shared hashes; a walk that ends before s


@pytest.mark.parametrize("s_ref,s_qry", [(1000, 64), (64, 1000), (65, 1), (1, 65)])
def test_tables_of_different_sketch_sizes(eng, s_ref, s_qry):
    rng = np.random.default_rng(s_ref)
    u = 3 * max(s_ref, s_qry)
    check_job(eng, make_table(rng, 9, s_ref, u, 1), make_table(rng, 11, s_qry, u, 1))


def test_rows_of_no_one_and_few_hashes(eng):
    rng = np.random.default_rng(3)
    exp = check_job(eng, make_table(rng, 12, 64, 90, 2), make_table(rng, 13, 64, 90, 2))
    assert (exp["denom"][0::3, :] == 0).all() and (exp["denom"][:, 0::3] == 0).all()      # empty rows: j = 0, never a line


def test_padding_never_matches_padding(eng):
    # two short rows share the padding value behind their hashes; a real hash equal to it is a member only where a row holds it
    ref = (np.array([[5, 9, PAD, PAD], [5, 9, PAD, PAD], [PAD, PAD, PAD, PAD]], dtype=np.uint64), np.array([2, 3, 0], dtype=np.uint32))
    qry = (np.array([[5, PAD, PAD, PAD, PAD, PAD], [9, PAD, PAD, PAD, PAD, PAD], [PAD] * 6, [1, 2, 3, 5, 9, 11]], dtype=np.uint64),
           np.array([1, 2, 1, 6], dtype=np.uint32))
    exp = check_job(eng, ref, qry)
    assert tuple(exp[0, 0]) == (1, 1) and tuple(exp[1, 0]) == (1, 1) and tuple(exp[1, 1]) == (2, 2)
    assert tuple(exp[2, 0]) == (0, 0) and tuple(exp[2, 1]) == (1, 1) and tuple(exp[3, 0]) == (0, 2)


def test_values_below_2_32(eng):
    rng = np.random.default_rng(4)
    check_job(eng, make_table(rng, 20, 64, 150, 1, limit=2 ** 32), make_table(rng, 20, 65, 150, 1, limit=2 ** 32))


@pytest.mark.parametrize("nref,nqry", [(1, 70), (70, 1), (1, 1)])
def test_one_reference_one_query(eng, nref, nqry):
    rng = np.random.default_rng(nref)
    check_job(eng, make_table(rng, nref, 64, 150, 1), make_table(rng, nqry, 64, 150, 1))


def test_query_ranges_and_device_blocks(eng):
    rng = np.random.default_rng(5)
    ref, qry = make_table(rng, 7, 65, 150, 1), make_table(rng, 33, 64, 150, 1)
    exp = expected(ref, qry)
    tr, tq = upload(eng, ref), upload(eng, qry)
    try:
        for knob in (None, 20):                                              # 20 pairs: blocks of two rows, 17 of them
            eng.set_option("MASHGPU_OUT_BLOCK_PAIRS", knob)
            for qb, qe in [(0, 33), (5, 6), (17, 33), (9, 9), (12, 5), (30, 1000), (40, 50)]:
                lo, hi = qb, max(qb, min(qe, 33))
                got = np.zeros((max(hi - lo, 0) + 1, 7), dtype=abi.COUNTS_DTYPE)
                got["numer"] = 0xABCD
                eng._check(eng.lib.mg_within_rect_host(eng.ctx, tr.handle, tq.handle, qb, qe, got.ctypes.data))
                assert np.array_equal(got[: hi - lo], exp[lo:hi]) and (got[hi - lo:]["numer"] == 0xABCD).all()      # nothing behind the range
                for e in (1.0, 0.2):
                    res = eng.within_rect_results(tr, tq, e, qb, qe)
                    assert np.array_equal(res, survivors(exp[lo:hi], e, lo)), (knob, qb, qe, e)
    finally:
        eng.set_option("MASHGPU_OUT_BLOCK_PAIRS", None)
        tr.free()
        tq.free()


def test_max_error_around_a_boundary_and_outside_0_1(eng):
    rng = np.random.default_rng(6)
    ref, qry = make_table(rng, 15, 64, 100, 1), make_table(rng, 17, 64, 100, 1)
    exp = expected(ref, qry)
    js = np.unique(exp["denom"])
    J = int(js[len(js) // 2])
    assert J > 1 and (exp["denom"] == J).any()
    at = 1.0 / math.sqrt(J)                                                   # passes J exactly
    below = math.nextafter(at, 0.0)                                           # J fails, the next j passes
    assert wm.j_min(at) == J and wm.j_min(below) == J + 1
    tr, tq = upload(eng, ref), upload(eng, qry)
    try:
        a, b = eng.within_rect_results(tr, tq, at), eng.within_rect_results(tr, tq, below)
        assert np.array_equal(a, survivors(exp, at)) and np.array_equal(b, survivors(exp, below))
        assert (a["denom"] == J).any() and not (b["denom"] == J).any() and len(b) == len(a) - int((exp["denom"] == J).sum())
        everything = survivors(exp, 1.0)
        assert len(everything) == int((exp["denom"] >= 1).sum())
        for e in (1.0, 1.5, math.inf):
            assert np.array_equal(eng.within_rect_results(tr, tq, e), everything)
        for e in (0.0, -0.5, -math.inf, math.nan):
            assert len(eng.within_rect_results(tr, tq, e)) == 0
        assert len(eng.within_rect_results(tr, tq, 0.01)) == 0                # j_min = 10 000 > s: no device work at all
        # the float conversion of the command line: (double)(float)0.125 == 0.125 = 1 / sqrt(64)
        assert np.array_equal(eng.within_rect_results(tr, tq, wm.as_float(0.125)), survivors(exp, 0.125))
    finally:
        tr.free()
        tq.free()


def test_capacity_protocol(eng):
    rng = np.random.default_rng(7)
    ref, qry = make_table(rng, 9, 64, 100, 1), make_table(rng, 11, 64, 100, 1)
    want = survivors(expected(ref, qry), 0.3)
    assert len(want) > 3
    tr, tq = upload(eng, ref), upload(eng, qry)
    try:
        call = lambda out, cap, n: eng.lib.mg_within_rect_results_host(eng.ctx, tr.handle, tq.handle, 0, 11, 0.3, out, cap, C.byref(n))
        n = C.c_uint64(0)
        assert call(None, 0, n) == abi.MG_ERR_NOMEM and n.value == len(want)         # the count alone
        small = np.zeros(len(want), dtype=abi.EDGE_DTYPE)
        n = C.c_uint64(0)
        assert call(small.ctypes.data, 3, n) == abi.MG_ERR_NOMEM and n.value == len(want)
        assert not small[3:].view(np.uint32).any()                                                   # nothing written past the capacity
        n = C.c_uint64(0)
        assert call(small.ctypes.data, len(want), n) == abi.MG_OK and n.value == len(want) and np.array_equal(small, want)
        n = C.c_uint64(77)
        assert eng.lib.mg_within_rect_results_host(eng.ctx, tr.handle, tq.handle, 4, 4, 0.3, None, 0, C.byref(n)) == abi.MG_OK and n.value == 0
        assert eng.lib.mg_within_rect_results_host(eng.ctx, tr.handle, tq.handle, 0, 11, 0.3, None, 5, C.byref(n)) == MG_ERR_INVALID
    finally:
        tr.free()
        tq.free()


# ------------------------------------------------------------------------------------------ through the command

META = wf.load_cases()


def mash(args, host_route, block_pairs=None):
    env = dict(os.environ)
    env.pop("MASH_AMD_HOST_FINISH", None)
    env.pop("MASH_AMD_BLOCK_PAIRS", None)
    if host_route:
        env["MASH_AMD_HOST_FINISH"] = "1"
    if block_pairs:
        env["MASH_AMD_BLOCK_PAIRS"] = str(block_pairs)
    return subprocess.run([MASH, *args], cwd=wf.DIR, capture_output=True, text=True, env=env, timeout=300)


@pytest.mark.parametrize("case", META["cases"], ids=[c["name"] for c in META["cases"]])
def test_command_prints_what_the_reference_printed(case):
    want = wf.recorded(case["name"])
    for host_route in (False, True):
        r = mash(case["cmd"], host_route)
        assert r.returncode == case["exit"], (host_route, r.stderr[-1000:])
        assert r.stdout == want, (host_route, r.stderr[-1000:])
    if case["name"].startswith("quirk"):
        assert "cannot be used when a sketch is provided" in r.stderr


def test_command_in_blocks_of_a_few_pairs():
    case = next(c for c in META["cases"] if c["name"] == "fa_e03")
    for host_route in (False, True):
        r = mash(case["cmd"], host_route, block_pairs=9)                     # 4 references: two queries a block
        assert r.returncode == 0 and r.stdout == wf.recorded("fa_e03"), (host_route, r.stderr[-1000:])
