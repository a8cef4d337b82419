"""`mash dist` (queries x references, mg_compare_rect_* and what is built on them) against the oracle.

The judge is helpers.rect_oracle (tests/test_rect_oracle.py checks it on the CPU), never another engine of this library.
Integers are compared exactly, distances exactly, p-values at the bar the project holds the oracle's log-space tail to
(1e-9 relative above 1e-290, <= 1e-280 below); the device finish against the host finish bit for bit.  Every call that
takes a query range gets every range of _ranges(): the rows of a result and its `row` fields are indices into the QUERY
TABLE (q_begin + local), and an empty range writes nothing."""
import ctypes as C

import numpy as np
import pytest

from mash_amd import abi
from tests import helpers
from tests.helpers import _check_records_against_oracle, _oracle_pass, _same_bits, _set_kernel

pytestmark = pytest.mark.gpu

K, KSPACE21 = 21, 4.0 ** 21
MG_ERR_INVALID, MG_ERR_UNSUPPORTED = -1, -2

SIZES = ((256, 128), (128, 256))                     # (s_ref, s_qry) of the unequal-size cases
COUNT_CASES = ["clean", "ragged"] + [f"{n}_{a}_{b}" for n in ("clean", "ragged") for a, b in SIZES]
ENGINES = ["default", "sparse", "merged", "plain", "generic", "windows29"]

# Cells (case, engine) where a FORCED engine may answer MG_ERR_UNSUPPORTED, with the library's own error text.  Only `join` and
# `windows*` cells may be listed, never join on species or windows29 on clean; every other refusal fails the test.
TOLERATED_REFUSALS = {}

FILTERS = ((0.1, -1.0), (-1.0, 1e-20), (0.3, 1e-5))
FINISH_SETTINGS = [(-1.0, -1.0), (1.0, 1.0), (0.2, -1.0), (-1.0, 1e-10), (0.08, 1e-30), (0.0, 1.0)]
SENTINEL = 0x5A5A5A5A


def _ranges(nq):
    """the whole table, the first and the last query, ranges across the 16-row plain tiles and the <= 32-row window tiles, one the
    library clamps, two empty ones"""
    return [(0, nq), (0, 1), (nq - 1, nq), (15, 17), (31, 65), (5, nq + 1000), (nq, nq), (40, 40)]


@pytest.fixture(scope="module")
def eng():
    import torch
    torch.cuda.init()          # (torch ships its own HIP runtime: it initialises first, tests/test_gpu_parity.py)
    e = abi.MashGpu(0)
    e.set_option("MASHGPU_COSTS_FIXED", "1")
    yield e
    e.close()


@pytest.fixture(scope="module")
def cases(oracle):
    """name -> the six arrays of a case, the oracle's [nq, nref] results and its counts as mg_counts; computed once, read-only"""
    out = {name: getattr(helpers, "rect_case_" + name)() for name in ("clean", "ragged", "species")}
    for name in ("clean", "ragged"):
        for a, b in SIZES:
            out[f"{name}_{a}_{b}"] = helpers.rect_case_sized(out[name], a, b)
    for name, c in out.items():
        c["numer"], c["denom"], c["dist"], c["pval"] = helpers.rect_case_oracle(oracle, c, K, KSPACE21)
        if name in ("clean", "ragged", "species"):
            helpers.check_rect_case_conditions(name, c, c["numer"], c["denom"])
        c["s"] = min(c["rt"].shape[1], c["qt"].shape[1])
        c["counts"] = np.zeros(c["numer"].shape, dtype=abi.COUNTS_DTYPE)
        c["counts"]["numer"], c["counts"]["denom"] = c["numer"], c["denom"]
        assert (c["numer"] >= 1).any() and (c["numer"] == 0).any()
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.flags.writeable = False
    # an unequal pair is another job than the equal sizes (and both pairs are ONE job to the oracle: s = 128 on both sides)
    assert not np.array_equal(out["clean"]["numer"], out["clean_256_128"]["numer"])
    assert np.array_equal(out["clean_256_128"]["numer"], out["clean_128_256"]["numer"])
    return out


@pytest.fixture(scope="module")
def tabs(eng, cases):
    t = {name: (eng.table_upload(c["rt"], c["rn"], c["rl"]), eng.table_upload(c["qt"], c["qn"], c["ql"])) for name, c in cases.items()}
    yield t
    for ref, qry in t.values():
        ref.free()
        qry.free()


@pytest.fixture(scope="module")
def host_fin(eng, cases):
    """mg_finish_rect_host of the ORACLE's counts of a whole case (every pair is finished on its own: a range is a slice)"""
    memo = {}

    def get(name, max_d, max_p):
        key = (name, max_d, max_p)
        if key not in memo:
            c = cases[name]
            memo[key] = eng.finish_rect(c["counts"], c["rl"], c["ql"], K, KSPACE21, max_d, max_p)
            memo[key].flags.writeable = False
        return memo[key]
    return get


def _clamp(qb, qe, nq):
    hi = min(qe, nq)
    return qb, hi, max(hi - qb, 0)


def _check_records_against_host(rec, host, max_d):
    assert np.array_equal(rec["numer"], host["numer"]) and np.array_equal(rec["denom"], host["denom"])
    assert np.array_equal(rec["pass"], host["pass"])
    assert _same_bits(rec["distance"], host["distance"])
    ok = host["pass"] == 1 if (0 <= max_d < 1) else np.ones(host.shape, dtype=bool)      # rejected by -d: only `pass` is meaningful
    assert _same_bits(rec["p_value"][ok], host["p_value"][ok])


def _survivors(c, host, lo, hi, max_d, max_p):
    """the oracle's passing pairs of queries [lo, hi), query major, as mg_result records with the host finish's doubles"""
    q, r = np.nonzero(_oracle_pass(c, max_d, max_p)[lo:hi])
    want = np.zeros(len(q), dtype=abi.RESULT_DTYPE)
    want["row"], want["col"] = q + lo, r
    want["numer"], want["denom"] = c["numer"][q + lo, r], c["denom"][q + lo, r]
    want["distance"], want["p_value"] = host["distance"][q + lo, r], host["p_value"][q + lo, r]
    assert np.all(host["pass"][q + lo, r] == 1) and int(host["pass"][lo:hi].sum()) == len(q)      # (the host finish agrees on who passes)
    return want


def _rect_host_guarded(eng, ref, qry, qb, qe, nq):
    """mg_compare_rect_host with the range as given (the library clamps) into a buffer with a guard row behind: (rc, rows written)"""
    lo, hi, rows = _clamp(qb, qe, nq)
    out = np.zeros((rows + 1, ref.rows), dtype=abi.COUNTS_DTYPE)
    out.view(np.uint32)[:] = SENTINEL
    rc = eng.lib.mg_compare_rect_host(eng.ctx, ref.handle, qry.handle, qb, qe, out.ctypes.data)
    assert np.all(out[rows:].view(np.uint32) == SENTINEL), "wrote past the range"
    if rc != abi.MG_OK:
        assert np.all(out.view(np.uint32) == SENTINEL)
    return rc, out[:rows]


# ------------------------------------------------------------------------------------------ 1. counts, every engine

@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", COUNT_CASES)
def test_rect_counts_every_engine_and_range(eng, cases, tabs, name, engine, monkeypatch):
    _set_kernel(monkeypatch, engine)
    c, (ref, qry) = cases[name], tabs[name]
    nq = len(c["qn"])
    for qb, qe in _ranges(nq):
        lo, hi, rows = _clamp(qb, qe, nq)
        rc, got = _rect_host_guarded(eng, ref, qry, qb, qe, nq)
        if rc == MG_ERR_UNSUPPORTED:
            msg = eng.lib.mg_last_error(eng.ctx).decode()
            assert engine.startswith("windows") and (name, engine) in TOLERATED_REFUSALS and name != "clean", (name, engine, qb, qe, msg)
            assert "cannot take" in msg and TOLERATED_REFUSALS[(name, engine)] in msg, msg
            continue
        assert rc == abi.MG_OK, (qb, qe, rc, eng.lib.mg_last_error(eng.ctx).decode())
        assert got.tobytes() == c["counts"][lo:hi].tobytes(), (name, engine, qb, qe)
    # the wrapper's form of the same call
    assert eng.compare_rect_host(ref, qry, 31, 65).tobytes() == c["counts"][31:65].tobytes()


def test_rect_counts_join_engine_on_one_species(eng, cases, tabs, monkeypatch):
    _set_kernel(monkeypatch, "join")
    c, (ref, qry) = cases["species"], tabs["species"]
    nq = len(c["qn"])
    eng.prof_enable(True)
    try:
        for qb, qe in ((0, nq), (15, 17), (31, nq + 1000), (nq, nq)):
            lo, hi, rows = _clamp(qb, qe, nq)
            eng.prof_reset()
            rc, got = _rect_host_guarded(eng, ref, qry, qb, qe, nq)
            assert rc == abi.MG_OK, (qb, qe, rc, eng.lib.mg_last_error(eng.ctx).decode())          # join never refuses species
            assert got.tobytes() == c["counts"][lo:hi].tobytes(), (qb, qe)
            assert eng.prof_avg_ms("compare_join")[1] >= (1 if rows else 0), (qb, qe)              # ... and it is the engine that ran
            assert rows or eng.prof_avg_ms("compare_join")[1] == 0
    finally:
        eng.prof_enable(False)


# ------------------------------------------------------------------------------------------ 2. mg_compare_rect_dev

def _counts_buffer(pairs):
    """a device buffer of pairs mg_counts with a guard record in front and two behind; the output starts 8 bytes in"""
    import torch
    return torch.full((pairs + 3, 2), SENTINEL, dtype=torch.int32, device="cuda")


def _check_counts_buffer(buf, want):
    dev = buf.cpu().numpy().view(np.uint32)
    pairs = want.size
    assert np.all(dev[0] == SENTINEL) and np.all(dev[pairs + 1:] == SENTINEL), "guard words overwritten"
    assert dev[1:pairs + 1].tobytes() == want.tobytes()


@pytest.mark.parametrize("engine", ["default", "sparse"])
@pytest.mark.parametrize("name", COUNT_CASES)
def test_rect_dev_synchronous_and_queued(eng, cases, tabs, name, engine, monkeypatch):
    import torch
    _set_kernel(monkeypatch, engine)
    c, (ref, qry) = cases[name], tabs[name]
    nq, nref = c["numer"].shape
    for qb, qe in _ranges(nq):
        lo, hi, rows = _clamp(qb, qe, nq)
        buf = _counts_buffer(rows * nref)
        torch.cuda.synchronize()
        eng.compare_rect_dev(ref, qry, qb, qe, buf.data_ptr() + 8)
        _check_counts_buffer(buf, c["counts"][lo:hi])
    # queued: three calls over different ranges into three buffers, one synchronisation
    three = [(31, 65), (0, nq), (5, nq + 1000)]
    bufs = [_counts_buffer(_clamp(qb, qe, nq)[2] * nref) for qb, qe in three]
    torch.cuda.synchronize()
    eng.set_async(True)
    try:
        for (qb, qe), buf in zip(three, bufs):
            eng.compare_rect_dev(ref, qry, qb, qe, buf.data_ptr() + 8)
        eng.synchronize()
    finally:
        eng.set_async(False)
    for (qb, qe), buf in zip(three, bufs):
        lo, hi, _ = _clamp(qb, qe, nq)
        _check_counts_buffer(buf, c["counts"][lo:hi])


# ------------------------------------------------------------------------------------------ 3. mg_finish_rect_dev

@pytest.mark.parametrize("max_d,max_p", FINISH_SETTINGS)
def test_finish_rect_dev_equals_host_finish_and_oracle(eng, cases, tabs, host_fin, max_d, max_p):
    import torch
    rec_bytes = abi.PAIR_DTYPE.itemsize
    for name in ("clean", "ragged", "clean_128_256"):
        c, (ref, qry) = cases[name], tabs[name]
        nq, nref = c["numer"].shape
        host = host_fin(name, max_d, max_p)
        _check_records_against_oracle(host, c, 0, nq, max_d, max_p)                     # the host finish itself
        for qb, qe in _ranges(nq):
            lo, hi, rows = _clamp(qb, qe, nq)
            pairs = rows * nref
            counts = _counts_buffer(pairs)
            out = torch.full(((pairs + 2) * rec_bytes,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            eng.compare_rect_dev(ref, qry, qb, qe, counts.data_ptr() + 8)
            eng.finish_rect_dev(ref, qry, counts.data_ptr() + 8, qb, qe, K, KSPACE21, max_d, max_p, out.data_ptr() + rec_bytes)
            eng.synchronize()
            _check_counts_buffer(counts, c["counts"][lo:hi])
            raw = out.cpu().numpy()
            assert np.all(raw[:rec_bytes] == 0xA5) and np.all(raw[(pairs + 1) * rec_bytes:] == 0xA5), "guard records overwritten"
            rec = raw[rec_bytes:(pairs + 1) * rec_bytes].view(abi.PAIR_DTYPE).reshape(rows, nref)
            _check_records_against_host(rec, host[lo:hi], max_d)                        # the output starts at q_begin
            _check_records_against_oracle(rec, c, lo, hi, max_d, max_p)


def test_finish_rect_dev_error_paths(eng, cases, tabs, host_fin):
    import torch
    c, (ref, qry) = cases["clean"], tabs["clean"]
    nq, nref = c["numer"].shape
    rec_bytes = abi.PAIR_DTYPE.itemsize
    counts = torch.from_numpy(c["counts"][:4].copy().view(np.uint32)).to("cuda")
    out = torch.full((4 * nref * rec_bytes,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def call(r, q, cp, op):
        return eng.lib.mg_finish_rect_dev(eng.ctx, r, q, cp, 0, 4, K, KSPACE21, -1.0, -1.0, op)

    assert call(None, qry.handle, counts.data_ptr(), out.data_ptr()) == MG_ERR_INVALID
    assert call(ref.handle, None, counts.data_ptr(), out.data_ptr()) == MG_ERR_INVALID
    assert call(ref.handle, qry.handle, None, out.data_ptr()) == MG_ERR_INVALID
    assert call(ref.handle, qry.handle, counts.data_ptr(), None) == MG_ERR_INVALID
    bare_q = eng.table_upload(c["qt"][:4], c["qn"][:4])                                 # tables without lengths
    bare_r = eng.table_upload(c["rt"], c["rn"])
    assert call(ref.handle, bare_q.handle, counts.data_ptr(), out.data_ptr()) == MG_ERR_INVALID
    assert "lengths" in eng.lib.mg_last_error(eng.ctx).decode()
    assert call(bare_r.handle, qry.handle, counts.data_ptr(), out.data_ptr()) == MG_ERR_INVALID
    bare_q.free()
    bare_r.free()
    eng.synchronize()
    assert np.all(out.cpu().numpy() == 0xA5)                                            # nothing was written on the way
    assert call(ref.handle, qry.handle, counts.data_ptr(), out.data_ptr()) == abi.MG_OK  # the context still works
    eng.synchronize()
    rec = out.cpu().numpy().view(abi.PAIR_DTYPE).reshape(4, nref)
    _check_records_against_host(rec, host_fin("clean", -1.0, -1.0)[:4], -1.0)


# ------------------------------------------------------------------------------------------ 4. pairs and results with ranges

@pytest.mark.parametrize("max_d,max_p", FILTERS)
@pytest.mark.parametrize("mode", ["lists", "matrix"])
def test_rect_pairs_and_results_with_ranges(eng, cases, tabs, host_fin, mode, max_d, max_p, monkeypatch):
    """mode lists: the inverted-index engine forced, so with a filter on the survivors come from the candidate lists (no matrix is
    filled: the counters say so on `clean`); mode matrix: MASHGPU_RESULTS_MATRIX=1, the matrix in blocks filtered on the device"""
    _set_kernel(monkeypatch, "sparse" if mode == "lists" else "default")
    if mode == "matrix":
        monkeypatch.setenv("MASHGPU_RESULTS_MATRIX", "1")
    for name in ("clean", "ragged", "clean_256_128", "clean_128_256", "ragged_128_256"):
        c, (ref, qry) = cases[name], tabs[name]
        nq, nref = c["numer"].shape
        host = host_fin(name, max_d, max_p)
        everyone = _survivors(c, host, 0, nq, max_d, max_p)
        assert 0 < len(everyone) < c["numer"].size and len(everyone) > 8
        for qb, qe in _ranges(nq):
            lo, hi, rows = _clamp(qb, qe, nq)
            pairs = eng.compare_rect_pairs(ref, qry, K, KSPACE21, max_d, max_p, q_begin=qb, q_end=qe)
            assert pairs.shape == (rows, nref)
            _check_records_against_host(pairs, host[lo:hi], max_d)
            _check_records_against_oracle(pairs, c, lo, hi, max_d, max_p)
            want = _survivors(c, host, lo, hi, max_d, max_p)
            counted = mode == "lists" and name.startswith("clean") and rows > 8
            if counted:
                eng.prof_enable(True)
                eng.prof_reset()
            got = eng.compare_rect_results(ref, qry, K, KSPACE21, max_d, max_p, q_begin=qb, q_end=qe)
            if counted:
                merged, filled = eng.prof_avg_ms("compare_merge")[1], eng.prof_avg_ms("compare_fill")[1]
                eng.prof_enable(False)
                assert merged >= 1 and filled == 0, (name, qb, qe, merged, filled)              # the list path really ran
            assert len(got) == len(want), (name, qb, qe)
            assert np.array_equal(got["row"], want["row"]) and np.array_equal(got["col"], want["col"]), (name, qb, qe)
            assert got.tobytes() == want.tobytes(), (name, qb, qe)
            if rows:
                assert len(want) == 0 or (int(got["row"].min()) >= lo and int(got["row"].max()) < hi)
        # a buffer that is too small: the count comes back, the second call fills it
        got = eng.compare_rect_results(ref, qry, K, KSPACE21, max_d, max_p, q_begin=5, q_end=nq + 1000, capacity=8)
        assert got.tobytes() == _survivors(c, host, 5, nq, max_d, max_p).tobytes()


# ------------------------------------------------------------------------------------------ 5. mg_compare_rect_sparse_host

@pytest.mark.parametrize("engine", ["sparse", "default"])
@pytest.mark.parametrize("name", COUNT_CASES + ["species"])
def test_rect_sparse_exceptions(eng, cases, tabs, name, engine, monkeypatch):
    _set_kernel(monkeypatch, engine)
    c, (ref, qry) = cases[name], tabs[name]
    nq, nref = c["numer"].shape
    for qb, qe in _ranges(nq):
        lo, hi, rows = _clamp(qb, qe, nq)
        want = helpers.edges_of(c["numer"][lo:hi], c["denom"][lo:hi], lo)
        counted = engine == "sparse" and name.startswith("clean") and rows > 8
        if counted:
            eng.prof_enable(True)
            eng.prof_reset()
        got = eng.compare_rect_sparse(ref, qry, qb, qe)
        if counted:
            merged, filled = eng.prof_avg_ms("compare_merge")[1], eng.prof_avg_ms("compare_fill")[1]
            eng.prof_enable(False)
            assert merged >= 1 and filled == 0, (name, qb, qe, merged, filled)                  # the lists, not the matrix
        assert len(got) == len(want), (name, engine, qb, qe, len(got), len(want))
        assert got.tobytes() == want.tobytes(), (name, engine, qb, qe)                          # row is absolute, col the reference
        key = got["row"].astype(np.int64) * nref + got["col"]
        assert np.all(np.diff(key) > 0)                                                         # strictly ascending (row, col)
        dense = helpers.expand_rect(got, c["rn"], c["qn"], c["s"], qb, qe, nref)
        assert dense.tobytes() == c["counts"][lo:hi].tobytes()
        assert dense.tobytes() == eng.compare_rect_host(ref, qry, qb, qe).tobytes()
    if name == "clean":                                                                         # shares a hash, numer 0: no exception
        q = c["where"]["behind_11"]
        whole = eng.compare_rect_sparse(ref, qry)
        assert not np.any((whole["row"] == q) & (whole["col"] == 11)) and np.any(whole["row"] == q + 1)


@pytest.mark.parametrize("engine", ["sparse", "default"])
@pytest.mark.parametrize("name", ["clean", "ragged"])
def test_rect_sparse_capacity_protocol_and_errors(eng, cases, tabs, name, engine, monkeypatch):
    _set_kernel(monkeypatch, engine)
    c, (ref, qry) = cases[name], tabs[name]
    qb, qe = 5, 70
    lo, hi, _ = _clamp(qb, qe, len(c["qn"]))
    want = helpers.edges_of(c["numer"][lo:hi], c["denom"][lo:hi], lo)
    n = C.c_uint64(0)

    def call(r, q, out, cap, cnt):
        return eng.lib.mg_compare_rect_sparse_host(eng.ctx, r, q, qb, qe, out, cap, cnt)

    assert call(ref.handle, qry.handle, None, 0, C.byref(n)) == abi.MG_ERR_NOMEM and n.value == len(want) > 1
    buf = np.zeros(len(want) + 1, dtype=abi.EDGE_DTYPE)
    buf.view(np.uint32)[:] = SENTINEL
    n.value = 0
    assert call(ref.handle, qry.handle, buf.ctypes.data, len(want) - 1, C.byref(n)) == abi.MG_ERR_NOMEM and n.value == len(want)
    assert np.all(buf[len(want) - 1:].view(np.uint32) == SENTINEL)
    assert call(ref.handle, qry.handle, buf.ctypes.data, len(want), C.byref(n)) == abi.MG_OK and n.value == len(want)
    assert buf[:len(want)].tobytes() == want.tobytes() and np.all(buf[len(want):].view(np.uint32) == SENTINEL)
    assert call(None, qry.handle, buf.ctypes.data, len(want), C.byref(n)) == MG_ERR_INVALID
    assert call(ref.handle, None, buf.ctypes.data, len(want), C.byref(n)) == MG_ERR_INVALID
    assert call(ref.handle, qry.handle, buf.ctypes.data, len(want), None) == MG_ERR_INVALID
    assert call(ref.handle, qry.handle, None, len(want), C.byref(n)) == MG_ERR_INVALID
    assert call(ref.handle, qry.handle, buf.ctypes.data, len(want), C.byref(n)) == abi.MG_OK and n.value == len(want)     # the context still works


# ------------------------------------------------------------------------------------------ 6. sharded, small

def test_sharded_rect_calls_equal_the_oracle(eng, cases, host_fin, monkeypatch):
    """mg_compare_rect_*_sharded_host over three contexts on one device, with query ranges: the reference replicated (the job is
    cut by reference rows: 1 200 references, 87 queries), replicated with the QUERIES cut (MASHGPU_RECT_SPLIT), and row-sharded"""
    c = cases["clean"]
    nq, nref = c["numer"].shape
    max_d, max_p = 0.3, 1e-5
    host = host_fin("clean", max_d, max_p)
    comm = abi.LocalComm([0, 0, 0])
    try:
        dq = comm.upload(c["qt"], c["qn"], c["ql"])
        for mode in ("replicated", "queries", "rows"):
            dr = comm.upload_rows(c["rt"], c["rn"], c["rl"]) if mode == "rows" else comm.upload(c["rt"], c["rn"], c["rl"])
            if mode == "queries":
                monkeypatch.setenv("MASHGPU_RECT_SPLIT", "queries")
            else:
                monkeypatch.delenv("MASHGPU_RECT_SPLIT", raising=False)
            for qb, qe in ((0, nq), (31, 65), (nq - 1, nq), (5, nq + 1000), (nq, nq)):
                lo, hi, rows = _clamp(qb, qe, nq)
                got = comm.rect(dr, dq, nref, nq, qb, hi)
                assert got.tobytes() == c["counts"][lo:hi].tobytes(), (mode, qb, qe)
                pairs = comm.rect_pairs(dr, dq, nref, nq, K, KSPACE21, max_d, max_p, q_begin=qb, q_end=qe)
                assert pairs.shape == (rows, nref)
                _check_records_against_host(pairs, host[lo:hi], max_d)
                _check_records_against_oracle(pairs, c, lo, hi, max_d, max_p)
                res = comm.rect_results(dr, dq, nq, K, KSPACE21, max_d, max_p, capacity=8, q_begin=qb, q_end=qe)
                assert res.tobytes() == _survivors(c, host, lo, hi, max_d, max_p).tobytes(), (mode, qb, qe)
            comm.free(dr)
        comm.free(dq)
    finally:
        comm.close()
