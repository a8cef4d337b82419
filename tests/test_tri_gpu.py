"""`mash triangle` (mg_compare_tri_* and what is built on them) over ROW RANGES against the oracle.

The judge is oracle.triangle (tests/test_tri_oracle.py checks its flat order and the helpers on the CPU), never another engine
of this library.  Integers are compared exactly, distances exactly, `pass` exactly against the oracle's two filters, p-values
at the bar the project holds the oracle's log-space tail to (1e-9 relative above 1e-290, <= 1e-280 below); the device finish
against mg_finish_tri_host of the ORACLE's counts bit for bit.  Whole arrays, never samples.  A range [rb, re) occupies pairs
[rb (rb - 1) / 2, re (re - 1) / 2) of the whole triangle; `row` and `col` of mg_edge / mg_result are indices into the TABLE; row 0
has no pair, row_end is clamped by the library, an empty range writes nothing and counts 0.

Two tables of 3 200 rows are the smallest on which a proper range still has 4 * 10^6 pairs: there the library serves a range
from a view of the table's first rows (host_compare.cpp: tri_view), builds the clustered index with a split at row_begin, and
the answer's ROUTE depends on the calls before it -- the answer must not."""
import ctypes as C
import os

import numpy as np
import pytest

from mash_amd import abi
from tests import helpers
from tests.helpers import _check_records_against_oracle, _oracle_pass, _same_bits, _set_kernel, tri_base

pytestmark = pytest.mark.gpu

K, KSPACE21 = 21, 4.0 ** 21
MG_ERR_INVALID, MG_ERR_UNSUPPORTED = -1, -2

SMALL = ("clades", "species", "ragged_head")
LARGE = ("families", "families_ragged")
ENGINES = ["default", "sparse", "merged", "plain", "generic", "join", "windows29"]

# Cells (case, engine) where a FORCED engine may answer MG_ERR_UNSUPPORTED, with the library's own error text.  Only `join` and
# `windows*` cells may be listed, never join on species; every other refusal fails the test.
TOLERATED_REFUSALS = {}

FINISH_SETTINGS = [(-1.0, -1.0), (1.0, 1.0), (0.2, -1.0), (-1.0, 1e-10), (0.08, 1e-30), (0.0, 1.0)]
# filters that are on: a share of the hit pairs strictly between none and all passes each (helpers.check_tri_case_conditions for
# the families; asserted on the oracle's output where they are used), and one that passes nothing
FILTERS = {"clades": ((0.0035, -1.0), (0.0045, 1e-30), (0.0, 1.0)),
           "families": ((0.05, 1e-30), (0.03, -1.0), (-1.0, 1e-30)),
           "families_ragged": ((0.05, 1e-30), (0.03, -1.0), (-1.0, 1e-30))}
SENTINEL = 0x5A5A5A5A

LARGE_RANGES = [(0, 3200),          # the whole triangle
                (0, 2900),          # the view's whole triangle
                (1000, 3100),       # view and split
                (2400, 3200),       # the table's last rows: no view, split
                (1500, 2000),       # below 4 * 10^6 pairs: no view, no index by default
                (3199, 4000), (0, 1), (3200, 3200)]


def _small_ranges(n):
    return [(0, n), (0, 1), (0, 2), (1, 2), (n - 1, n), (15, 17), (31, 65), (5, n + 1000), (n, n), (40, 40)]


def _ranges(name, c):
    if name in LARGE:
        return LARGE_RANGES
    out = _small_ranges(c["n"])
    if name == "clades":
        spans = c["where"]["clades"]
        (a0, b0), (a2, b2) = spans[0], spans[2]
        inside, last_in, first_in = (a2 + 15, b2 - 100), (b0 + 1, a2 + 65), (b2 - 35, b2 + 2)
        assert a2 <= inside[0] and inside[1] <= b2                                          # wholly inside one clade
        assert b0 <= last_in[0] < spans[1][0] and a2 <= last_in[1] - 1 < b2                 # first row between clades, last row inside
        assert a2 <= first_in[0] < b2 <= first_in[1] - 1 < spans[3][0]                      # first row inside, last row between
        out = out + [inside, last_in, first_in]
    return out


def _clamp(rb, re, n):
    """(first pair, one past the last pair, pairs) of rows [rb, min(re, n)) in the whole triangle's flat arrays"""
    hi = min(re, n)
    if rb >= hi:
        return tri_base(rb), tri_base(rb), 0
    return tri_base(rb), tri_base(hi), tri_base(hi) - tri_base(rb)


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
    """name -> table, nhash, lengths, the oracle's flat numer / denom / dist / pval and its counts as mg_counts; once, read-only"""
    out = {name: getattr(helpers, "tri_case_" + name)() for name in ("clades", "species", "families", "families_ragged")}
    out["ragged_head"] = helpers.tri_case_head(out["families_ragged"], 600)
    for name, c in out.items():
        c["numer"], c["denom"], c["dist"], c["pval"] = helpers.tri_case_oracle(oracle, c, K, KSPACE21)
        if name != "ragged_head":
            helpers.check_tri_case_conditions(name, c, c["numer"], c["denom"], c["dist"], c["pval"])
        c["counts"] = np.zeros(len(c["numer"]), dtype=abi.COUNTS_DTYPE)
        c["counts"]["numer"], c["counts"]["denom"] = c["numer"], c["denom"]
        assert (c["numer"] >= 1).any() and (name == "species" or (c["numer"] == 0).any())
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.flags.writeable = False
    # a head of a table is a prefix of its triangle
    assert np.array_equal(out["ragged_head"]["numer"], out["families_ragged"]["numer"][:tri_base(600)])
    for name, filters in FILTERS.items():
        hit = out[name]["numer"] >= 1
        for max_d, max_p in filters[:-1] if name == "clades" else filters:
            passing = int((_oracle_pass(out[name], max_d, max_p) & hit).sum())
            assert 0.05 * hit.sum() < passing < 0.95 * hit.sum(), (name, max_d, max_p, passing, int(hit.sum()))
    return out


@pytest.fixture(scope="module")
def tabs(eng, cases):
    t = {name: eng.table_upload(c["table"], c["nhash"], c["lengths"]) for name, c in cases.items()}
    yield t
    for tab in t.values():
        tab.free()


@pytest.fixture(scope="module")
def host_fin(eng, cases):
    """mg_finish_tri_host of the ORACLE's counts of a whole case (every pair is finished on its own: a range is a slice), held to
    the oracle's distances, filters and p-values before anything is compared with it"""
    memo = {}

    def get(name, max_d, max_p):
        key = (name, max_d, max_p)
        if key not in memo:
            if name in LARGE and sum(1 for k in memo if k[0] in LARGE) >= 4:                   # (160 MB each)
                for k in [k for k in memo if k[0] in LARGE]:
                    del memo[k]
            c = cases[name]
            fin = eng.finish_tri(c["counts"], c["lengths"], 0, c["n"], K, KSPACE21, max_d, max_p)
            _check_records_against_oracle(fin, c, 0, len(fin), max_d, max_p)
            fin.flags.writeable = False
            memo[key] = fin
        return memo[key]
    return get


def _check_records_against_host(rec, host, max_d):
    assert np.array_equal(rec["numer"], host["numer"]) and np.array_equal(rec["denom"], host["denom"])
    assert np.array_equal(rec["pass"], host["pass"])
    assert _same_bits(rec["distance"], host["distance"])
    ok = host["pass"] == 1 if (0 <= max_d < 1) else np.ones(host.shape, dtype=bool)      # rejected by -d: only `pass` is meaningful
    assert _same_bits(rec["p_value"][ok], host["p_value"][ok])


def _survivors(c, host, rb, re, max_d, max_p):
    """the oracle's passing pairs of rows [rb, re), reference order, as mg_result records (row, col: table indices) with the host
    finish's doubles"""
    lo, hi, pairs = _clamp(rb, re, c["n"])
    at = np.nonzero(_oracle_pass(c, max_d, max_p)[lo:hi])[0]
    rows, cols = helpers.tri_rows_cols(rb, min(re, c["n"]))
    want = np.zeros(len(at), dtype=abi.RESULT_DTYPE)
    want["row"], want["col"] = rows[at], cols[at]
    want["numer"], want["denom"] = c["numer"][lo:hi][at], c["denom"][lo:hi][at]
    want["distance"], want["p_value"] = host["distance"][lo:hi][at], host["p_value"][lo:hi][at]
    assert np.all(host["pass"][lo:hi][at] == 1) and int(host["pass"][lo:hi].sum()) == len(at)      # (the host finish agrees on who passes)
    assert len(at) == 0 or (int(want["row"].min()) >= rb and np.all(want["col"] < want["row"]))
    return want


def _tri_host_guarded(eng, tab, rb, re, n):
    """mg_compare_tri_host with the range as given (the library clamps) into a buffer with guard records behind: (rc, pairs written)"""
    lo, hi, pairs = _clamp(rb, re, n)
    out = np.empty(pairs + 2, dtype=abi.COUNTS_DTYPE)
    out.view(np.uint32)[:] = SENTINEL
    rc = eng.lib.mg_compare_tri_host(eng.ctx, tab.handle, rb, re, out.ctypes.data)
    assert np.all(out[pairs:].view(np.uint32) == SENTINEL), "wrote past the range"
    if rc != abi.MG_OK:
        assert np.all(out.view(np.uint32) == SENTINEL)
    return rc, out[:pairs]


def _check_counts(got, c, rb, re, what):
    lo, hi, _ = _clamp(rb, re, c["n"])
    want = c["counts"][lo:hi]
    if got.tobytes() != want.tobytes():
        bad = np.nonzero((got["numer"] != want["numer"]) | (got["denom"] != want["denom"]))[0]
        rows, cols = helpers.tri_rows_cols(rb, min(re, c["n"]))
        first = [(int(rows[i]), int(cols[i]), tuple(got[i]), tuple(want[i])) for i in bad[:5]]
        raise AssertionError(f"{what} rows [{rb}, {re}): {len(bad)} of {len(want)} pairs differ from the oracle; (row, col, got, want): {first}")


# ------------------------------------------------------------------------------------------ 1. counts, every engine

# (MASHGPU_COMPARE_DENSE is a knob of the index engine: off with the two engines that may build one)
@pytest.mark.parametrize("name,engine,dense", [(n, e, "on") for n in SMALL for e in ENGINES] +
                         [(n, e, "off") for n in SMALL for e in ("default", "sparse")])
def test_tri_counts_every_engine_and_range(eng, cases, tabs, name, engine, dense, monkeypatch):
    _set_kernel(monkeypatch, engine)
    if dense == "off":
        monkeypatch.setenv("MASHGPU_COMPARE_DENSE", "0")
    c, tab = cases[name], tabs[name]
    n = c["n"]
    tab.invalidate()
    eng.prof_enable(True)
    try:
        for rb, re in _ranges(name, c):
            eng.prof_reset()
            rc, got = _tri_host_guarded(eng, tab, rb, re, n)
            if rc == MG_ERR_UNSUPPORTED:
                msg = eng.lib.mg_last_error(eng.ctx).decode()
                assert (engine == "join" or engine.startswith("windows")) and (name, engine) in TOLERATED_REFUSALS, (name, engine, rb, re, msg)
                assert (name, engine) != ("species", "join") and TOLERATED_REFUSALS[(name, engine)] in msg, msg
                continue
            assert rc == abi.MG_OK, (rb, re, rc, eng.lib.mg_last_error(eng.ctx).decode())
            _check_counts(got, c, rb, re, (name, engine, dense))
            whole = (rb, re) == (0, n)
            if whole and name == "clades" and engine == "sparse":                 # the clades' inner pairs went through the dense kernel
                assert (eng.prof_avg_ms("compare_dense")[1] >= 1) == (dense == "on")
            if whole and name == "species" and engine == "join":                  # ... and the join engine is the one that ran
                assert eng.prof_avg_ms("compare_join")[1] >= 1
    finally:
        eng.prof_enable(False)
    # the wrapper's form of the same call
    lo, hi, _ = _clamp(31, 65, n)
    assert eng.compare_tri_host(tab, 31, 65).tobytes() == c["counts"][lo:hi].tobytes()


# ------------------------------------------------------------------------------------------ 2. mg_compare_tri_dev

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
@pytest.mark.parametrize("name", ["clades", "families"])
def test_tri_dev_writes_its_range_and_nothing_else(eng, cases, tabs, name, engine, monkeypatch):
    import torch
    _set_kernel(monkeypatch, engine)
    c, tab = cases[name], tabs[name]
    tab.invalidate()
    for rb, re in _ranges(name, c):
        lo, hi, pairs = _clamp(rb, re, c["n"])
        buf = _counts_buffer(pairs)
        torch.cuda.synchronize()
        eng.compare_tri_dev(tab, rb, re, buf.data_ptr() + 8)
        _check_counts_buffer(buf, c["counts"][lo:hi])                       # (an empty range and rows [0, 1): guards only)


def test_tri_dev_fill_beside_the_index_build_on_a_range(eng, cases, monkeypatch):
    """the constant written on a second stream while the index is built (SparseJobRun::prefill), on a range whose output does not
    begin at pair 0 of the triangle"""
    import torch
    monkeypatch.setenv("MASHGPU_FILL_ASIDE_MIN_PAIRS", "1")
    c = cases["families"]
    rb, re = 1000, 3100
    lo, hi, pairs = _clamp(rb, re, c["n"])
    tab = eng.table_upload(c["table"], c["nhash"], c["lengths"])          # fresh: no index yet
    buf = _counts_buffer(pairs)
    torch.cuda.synchronize()
    eng.prof_enable(True)
    eng.prof_reset()
    try:
        eng.compare_tri_dev(tab, rb, re, buf.data_ptr() + 8)
        aside = eng.prof_avg_ms("compare_fill_aside")[1]
    finally:
        eng.prof_enable(False)
    _check_counts_buffer(buf, c["counts"][lo:hi])
    assert aside >= 1                                                       # the fill beside the build is what ran
    tab.free()


# ------------------------------------------------------------------------------------------ 3. the 3 200-row tables

@pytest.mark.parametrize("knob", ["none", "MASHGPU_SPLIT_ALWAYS=1", "MASHGPU_TRI_PREFIX=0", "MASHGPU_COMPARE_CLUSTER=0"])
@pytest.mark.parametrize("engine", ["default", "sparse"])
@pytest.mark.parametrize("name", LARGE)
def test_tri_counts_views_split_and_clustered_index(eng, cases, tabs, name, engine, knob, monkeypatch):
    """every range on its own (mg_table_invalidate before it): served from a view of the first rows, from the clustered index with
    a split at row_begin (MASHGPU_SPLIT_ALWAYS: at s = 64 the size rule keeps the table's order otherwise), or with either off"""
    _set_kernel(monkeypatch, engine)
    if knob != "none":
        monkeypatch.setenv(*knob.split("="))
    c, tab = cases[name], tabs[name]
    eng.prof_enable(True)
    try:
        for rb, re in LARGE_RANGES:
            tab.invalidate()
            eng.prof_reset()
            rc, got = _tri_host_guarded(eng, tab, rb, re, c["n"])
            assert rc == abi.MG_OK, (rb, re, rc, eng.lib.mg_last_error(eng.ctx).decode())
            _check_counts(got, c, rb, re, (name, engine, knob))
            if knob == "MASHGPU_SPLIT_ALWAYS=1" and engine == "sparse" and name == "families" and (rb, re) in ((2400, 3200), (1000, 3100)):
                # the rows of a family are neighbours inside each segment of the split order: the dense kernel ran
                assert eng.prof_avg_ms("compare_dense")[1] >= 1, (rb, re)
    finally:
        eng.prof_enable(False)
        tab.invalidate()


# ------------------------------------------------------------------------------------------ 4. the view depends on history

HISTORY = [(1000, 3100),        # makes a view of the first 3 100 rows
           (0, 2900),           # served by that view
           (500, 3150),         # covered by no view: the whole table
           (1000, 3100),        # now served by the whole table's index
           None,                # mg_table_invalidate
           (0, 2900)]           # ... and first


@pytest.mark.parametrize("form", ["counts", "results"])
def test_tri_answers_do_not_depend_on_the_calls_before(eng, cases, host_fin, form):
    c = cases["families"]
    max_d, max_p = FILTERS["families"][0]
    tab = eng.table_upload(c["table"], c["nhash"], c["lengths"])           # fresh: no view, no index
    for step, r in enumerate(HISTORY):
        if r is None:
            tab.invalidate()
            continue
        rb, re = r
        if form == "counts":
            rc, got = _tri_host_guarded(eng, tab, rb, re, c["n"])
            assert rc == abi.MG_OK, (step, rc, eng.lib.mg_last_error(eng.ctx).decode())
            _check_counts(got, c, rb, re, ("history", step))
        else:
            want = _survivors(c, host_fin("families", max_d, max_p), rb, re, max_d, max_p)
            got = eng.compare_tri_results(tab, K, KSPACE21, max_d, max_p, row_begin=rb, row_end=re)
            assert len(got) == len(want) > 1000, (step, rb, re, len(got), len(want))
            assert np.array_equal(got["row"], want["row"]) and np.array_equal(got["col"], want["col"]), (step, rb, re)
            assert got.tobytes() == want.tobytes(), (step, rb, re)
    tab.free()


# ------------------------------------------------------------------------------------------ 5. mg_finish_tri_dev

@pytest.mark.parametrize("max_d,max_p", FINISH_SETTINGS)
def test_finish_tri_dev_equals_host_finish_and_oracle(eng, cases, tabs, host_fin, max_d, max_p):
    import torch
    rec_bytes = abi.PAIR_DTYPE.itemsize
    for name in ("clades", "ragged_head"):
        c, tab = cases[name], tabs[name]
        host = host_fin(name, max_d, max_p)
        for rb, re in _ranges(name, c):
            lo, hi, pairs = _clamp(rb, re, c["n"])
            counts = _counts_buffer(pairs)
            out = torch.full(((pairs + 2) * rec_bytes,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            eng.compare_tri_dev(tab, rb, re, counts.data_ptr() + 8)
            eng.finish_tri_dev(tab, counts.data_ptr() + 8, rb, re, K, KSPACE21, max_d, max_p, out.data_ptr() + rec_bytes)
            eng.synchronize()
            _check_counts_buffer(counts, c["counts"][lo:hi])
            raw = out.cpu().numpy()
            assert np.all(raw[:rec_bytes] == 0xA5) and np.all(raw[(pairs + 1) * rec_bytes:] == 0xA5), "guard records overwritten"
            rec = raw[rec_bytes:(pairs + 1) * rec_bytes].view(abi.PAIR_DTYPE)
            _check_records_against_host(rec, host[lo:hi], max_d)                        # the output starts at row_begin
            _check_records_against_oracle(rec, c, lo, hi, max_d, max_p)


def test_finish_tri_dev_error_paths(eng, cases, tabs, host_fin):
    import torch
    c, tab = cases["clades"], tabs["clades"]
    rb, re = 31, 65
    lo, hi, pairs = _clamp(rb, re, c["n"])
    rec_bytes = abi.PAIR_DTYPE.itemsize
    counts = torch.from_numpy(c["counts"][lo:hi].copy().view(np.uint32)).to("cuda")
    out = torch.full((pairs * rec_bytes,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def call(t, cp, op, b=rb, e=re):
        return eng.lib.mg_finish_tri_dev(eng.ctx, t, cp, b, e, K, KSPACE21, -1.0, -1.0, op)

    assert call(None, counts.data_ptr(), out.data_ptr()) == MG_ERR_INVALID
    assert call(tab.handle, None, out.data_ptr()) == MG_ERR_INVALID
    assert call(tab.handle, counts.data_ptr(), None) == MG_ERR_INVALID
    bare = eng.table_upload(c["table"], c["nhash"])                                     # a table without lengths
    assert call(bare.handle, counts.data_ptr(), out.data_ptr()) == MG_ERR_INVALID
    assert "lengths" in eng.lib.mg_last_error(eng.ctx).decode()
    bare.free()
    for b, e in ((0, 1), (c["n"], c["n"]), (40, 40), (c["n"] + 5, c["n"] + 9)):        # no pair: MG_OK, nothing written
        assert call(tab.handle, counts.data_ptr(), out.data_ptr(), b, e) == abi.MG_OK
    eng.synchronize()
    assert np.all(out.cpu().numpy() == 0xA5)                                            # nothing was written on the way
    assert call(tab.handle, counts.data_ptr(), out.data_ptr()) == abi.MG_OK             # the context still works
    eng.synchronize()
    rec = out.cpu().numpy().view(abi.PAIR_DTYPE)
    _check_records_against_host(rec, host_fin("clades", -1.0, -1.0)[lo:hi], -1.0)


# ------------------------------------------------------------------------------------------ 6. pairs and results with ranges

def _set_mode(monkeypatch, mode):
    _set_kernel(monkeypatch, "sparse" if mode == "sparse" else "default")
    if mode == "matrix":
        monkeypatch.setenv("MASHGPU_RESULTS_MATRIX", "1")


def _results_direct(eng, tab, rb, re, max_d, max_p, buf, capacity, k=K):
    n = C.c_uint64(0xDEAD)
    rc = eng.lib.mg_compare_tri_results_host(eng.ctx, tab.handle, rb, re, k, KSPACE21, max_d, max_p,
                                             None if buf is None else buf.ctypes.data, capacity, C.byref(n))
    return rc, n.value


def _pairs_and_results(eng, c, tab, host, ranges, max_d, max_p, protocol_range):
    for rb, re in ranges:
        lo, hi, npairs = _clamp(rb, re, c["n"])
        # every pair: through the library's own clamp, into a buffer sized for the clamped range with a guard record behind
        rec = np.empty(npairs + 1, dtype=abi.PAIR_DTYPE)
        rec.view(np.uint8)[:] = 0xA5
        rc = eng.lib.mg_compare_tri_pairs_host(eng.ctx, tab.handle, rb, re, K, KSPACE21, max_d, max_p, rec.ctypes.data)
        assert rc == abi.MG_OK, (rb, re, rc, eng.lib.mg_last_error(eng.ctx).decode())
        assert np.all(rec[npairs:].view(np.uint8) == 0xA5), "wrote past the range"
        _check_records_against_host(rec[:npairs], host[lo:hi], max_d)
        _check_records_against_oracle(rec[:npairs], c, lo, hi, max_d, max_p)
        # the survivors
        want = _survivors(c, host, rb, re, max_d, max_p)
        buf = np.empty(len(want) + 1, dtype=abi.RESULT_DTYPE)
        buf.view(np.uint8)[:] = 0xA5
        rc, count = _results_direct(eng, tab, rb, re, max_d, max_p, buf, len(want))
        assert rc == abi.MG_OK and count == len(want), (rb, re, rc, count, len(want), eng.lib.mg_last_error(eng.ctx).decode())
        got = buf[:count]
        assert np.all(buf[count:].view(np.uint8) == 0xA5), "wrote past the survivors"
        assert np.array_equal(got["row"], want["row"]) and np.array_equal(got["col"], want["col"]), (rb, re)
        assert got.tobytes() == want.tobytes(), (rb, re)
    # a buffer one record short: MG_ERR_NOMEM and the true count; the count alone; then the retry
    rb, re = protocol_range
    want = _survivors(c, host, rb, re, max_d, max_p)
    assert len(want) >= 2
    buf = np.zeros(len(want), dtype=abi.RESULT_DTYPE)
    assert _results_direct(eng, tab, rb, re, max_d, max_p, buf, len(want) - 1) == (abi.MG_ERR_NOMEM, len(want))
    assert _results_direct(eng, tab, rb, re, max_d, max_p, None, 0) == (abi.MG_ERR_NOMEM, len(want))
    assert _results_direct(eng, tab, rb, re, max_d, max_p, buf, len(want)) == (abi.MG_OK, len(want))
    assert buf.tobytes() == want.tobytes()
    # the wrapper's form (it sizes the buffer by a first call)
    assert eng.compare_tri_results(tab, K, KSPACE21, max_d, max_p, row_begin=rb, row_end=re, capacity=8).tobytes() == want.tobytes()
    lo, hi, _ = _clamp(rb, re, c["n"])
    _check_records_against_host(eng.compare_tri_pairs(tab, K, KSPACE21, max_d, max_p, row_begin=rb, row_end=re), host[lo:hi], max_d)
    n = c["n"]                                                                           # ... which clamps row_end itself
    rec = eng.compare_tri_pairs(tab, K, KSPACE21, max_d, max_p, row_begin=n - 3, row_end=n + 10 ** 6)
    assert len(rec) == tri_base(n) - tri_base(n - 3)
    _check_records_against_host(rec, host[tri_base(n - 3):], max_d)


@pytest.mark.parametrize("fi", [0, 1, 2])
@pytest.mark.parametrize("mode", ["default", "sparse", "matrix"])
def test_tri_pairs_and_results_with_ranges_small(eng, cases, tabs, host_fin, mode, fi, monkeypatch):
    _set_mode(monkeypatch, mode)
    c, tab = cases["clades"], tabs["clades"]
    max_d, max_p = FILTERS["clades"][fi]
    host = host_fin("clades", max_d, max_p)
    if fi == 2:                                                                          # nothing passes: no copy among the rows
        assert int(host["pass"].sum()) == 0
        for rb, re in _ranges("clades", c):
            assert _results_direct(eng, tab, rb, re, max_d, max_p, None, 0) == (abi.MG_OK, 0), (rb, re)
        return
    _pairs_and_results(eng, c, tab, host, _ranges("clades", c), max_d, max_p, (31, 65))


@pytest.mark.parametrize("fi", [0, 1])
@pytest.mark.parametrize("mode", ["default", "sparse", "matrix"])
@pytest.mark.parametrize("name", LARGE)
def test_tri_pairs_and_results_with_ranges_large(eng, cases, tabs, host_fin, name, mode, fi, monkeypatch):
    _set_mode(monkeypatch, mode)
    c, tab = cases[name], tabs[name]
    tab.invalidate()
    max_d, max_p = FILTERS[name][fi]
    _pairs_and_results(eng, c, tab, host_fin(name, max_d, max_p), LARGE_RANGES, max_d, max_p, (1000, 3100))
    tab.invalidate()


def test_tri_and_rect_pairs_and_results_error_paths(eng, cases, tabs):
    """k = 0, and a table uploaded without lengths: mg_table_upload keeps an array of zeros for it, which is no length to finish
    a p-value with (include/mashgpu.h: "the tables must carry lengths")"""
    c, tab = cases["clades"], tabs["clades"]
    rb, re = 31, 65
    _, _, pairs = _clamp(rb, re, c["n"])
    rec = np.zeros(max(pairs, (re - rb) * c["n"]), dtype=abi.PAIR_DTYPE)
    res = np.zeros(len(rec), dtype=abi.RESULT_DTYPE)
    n = C.c_uint64(0)
    lib, ctx = eng.lib, eng.ctx

    def tri_pairs(t, k=K):
        return lib.mg_compare_tri_pairs_host(ctx, t.handle, rb, re, k, KSPACE21, 0.1, 1e-10, rec.ctypes.data)

    def tri_results(t, k=K):
        return lib.mg_compare_tri_results_host(ctx, t.handle, rb, re, k, KSPACE21, 0.1, 1e-10, res.ctypes.data, len(res), C.byref(n))

    def rect_pairs(r, q):
        return lib.mg_compare_rect_pairs_host(ctx, r.handle, q.handle, rb, re, K, KSPACE21, 0.1, 1e-10, rec.ctypes.data)

    def rect_results(r, q):
        return lib.mg_compare_rect_results_host(ctx, r.handle, q.handle, rb, re, K, KSPACE21, 0.1, 1e-10, res.ctypes.data, len(res), C.byref(n))

    assert tri_pairs(tab, k=0) == MG_ERR_INVALID and tri_results(tab, k=0) == MG_ERR_INVALID
    bare = eng.table_upload(c["table"], c["nhash"])
    for call in (lambda: tri_pairs(bare), lambda: tri_results(bare), lambda: rect_pairs(bare, tab), lambda: rect_pairs(tab, bare),
                 lambda: rect_results(bare, tab), lambda: rect_results(tab, bare)):
        assert call() == MG_ERR_INVALID
        assert "lengths" in lib.mg_last_error(ctx).decode()
    assert lib.mg_compare_tri_host(ctx, bare.handle, rb, re, rec.ctypes.data) == abi.MG_OK       # counts need no lengths
    bare.free()
    assert tri_pairs(tab) == abi.MG_OK and tri_results(tab) == abi.MG_OK and n.value > 0         # the context still works
    assert rect_pairs(tab, tab) == abi.MG_OK and rect_results(tab, tab) == abi.MG_OK


def test_sharded_pairs_and_results_refuse_a_table_without_lengths(cases):
    c = cases["clades"]
    comm = abi.LocalComm([0, 0])
    try:
        d = comm.upload(c["table"], c["nhash"], c["lengths"])
        bare = C.c_void_p()
        comm._check(comm.lib.mg_dtable_upload(comm.h, c["table"].ctypes.data, c["nhash"].ctypes.data, None, c["n"], c["s"], C.byref(bare)))
        rec = np.zeros(c["n"] * c["n"], dtype=abi.PAIR_DTYPE)             # (room for what a call that wrongly succeeds would write)
        res = np.zeros(1 << 16, dtype=abi.RESULT_DTYPE)
        n = C.c_uint64(0)
        for rb, re in ((0, c["n"]), (31, 65)):                    # (every device's block is refused, the last ones included)
            assert comm.lib.mg_compare_tri_pairs_sharded_host(comm.h, bare, rb, re, K, KSPACE21, 0.1, 1e-10, rec.ctypes.data) == MG_ERR_INVALID
            assert "lengths" in comm.lib.mg_comm_last_error(comm.h).decode()
            assert comm.lib.mg_compare_tri_results_sharded_host(comm.h, bare, rb, re, K, KSPACE21, 0.1, 1e-10, res.ctypes.data, len(res), C.byref(n)) == MG_ERR_INVALID
            assert comm.lib.mg_compare_rect_pairs_sharded_host(comm.h, bare, d, rb, re, K, KSPACE21, 0.1, 1e-10, rec.ctypes.data) == MG_ERR_INVALID
            assert comm.lib.mg_compare_rect_results_sharded_host(comm.h, d, bare, rb, re, K, KSPACE21, 0.1, 1e-10, res.ctypes.data, len(res), C.byref(n)) == MG_ERR_INVALID
        lo, hi, _ = _clamp(31, 65, c["n"])
        assert comm.tri(bare, c["n"], 31, 65).tobytes() == c["counts"][lo:hi].tobytes()          # counts need no lengths
        comm.free(bare)
        comm.free(d)
    finally:
        comm.close()


# ------------------------------------------------------------------------------------------ 7. mg_compare_tri_filter_host

def _filter_direct(eng, tab, rb, re, max_d, buf, capacity):
    n = C.c_uint64(0xDEAD)
    rc = eng.lib.mg_compare_tri_filter_host(eng.ctx, tab.handle, rb, re, K, max_d, None if buf is None else buf.ctypes.data, capacity, C.byref(n))
    return rc, n.value


def _filter_want(c, rb, re, max_d):
    lo, hi, _ = _clamp(rb, re, c["n"])
    at = np.nonzero(c["dist"][lo:hi] <= max_d)[0]
    rows, cols = helpers.tri_rows_cols(rb, min(re, c["n"]))
    want = np.zeros(len(at), dtype=abi.EDGE_DTYPE)
    want["row"], want["col"], want["numer"], want["denom"] = rows[at], cols[at], c["numer"][lo:hi][at], c["denom"][lo:hi][at]
    return want


@pytest.mark.parametrize("engine", ["default", "sparse"])
@pytest.mark.parametrize("name,max_d", [("clades", 0.0), ("clades", 0.0035), ("clades", 0.3), ("clades", 1.0),
                                        ("families", 0.0), ("families", 0.03), ("families", 1.0),
                                        ("families_ragged", 0.0), ("families_ragged", 0.05), ("families_ragged", 1.0)])
def test_tri_filter_with_ranges(eng, cases, tabs, name, max_d, engine, monkeypatch):
    _set_kernel(monkeypatch, engine)
    c, tab = cases[name], tabs[name]
    tab.invalidate()
    everyone = int((c["dist"] <= max_d).sum())
    if max_d == 1.0:
        assert everyone == len(c["dist"])
    elif max_d == 0.0:
        assert everyone == (0 if name != "families_ragged" else 3)                    # (its two copied rows, and empty against empty)
    else:
        assert 0 < everyone < len(c["dist"])
    for rb, re in _ranges(name, c):
        want = _filter_want(c, rb, re, max_d)
        buf = np.empty(len(want) + 1, dtype=abi.EDGE_DTYPE)
        buf.view(np.uint32)[:] = SENTINEL
        rc, count = _filter_direct(eng, tab, rb, re, max_d, buf, len(want))
        assert rc == abi.MG_OK and count == len(want), (rb, re, rc, count, len(want), eng.lib.mg_last_error(eng.ctx).decode())
        assert np.all(buf[count:].view(np.uint32) == SENTINEL), "wrote past the survivors"
        assert buf[:count].tobytes() == want.tobytes(), (rb, re)
    rb, re = (31, 65) if name == "clades" else (1000, 3100)
    want = _filter_want(c, rb, re, max_d)
    if len(want) >= 2:
        buf = np.zeros(len(want), dtype=abi.EDGE_DTYPE)
        assert _filter_direct(eng, tab, rb, re, max_d, buf, len(want) - 1) == (abi.MG_ERR_NOMEM, len(want))
        assert _filter_direct(eng, tab, rb, re, max_d, None, 0) == (abi.MG_ERR_NOMEM, len(want))
        assert _filter_direct(eng, tab, rb, re, max_d, buf, len(want)) == (abi.MG_OK, len(want))
        assert buf.tobytes() == want.tobytes()
    else:
        assert _filter_direct(eng, tab, rb, re, max_d, None, 0) == (abi.MG_OK, 0)
    tab.invalidate()


# ------------------------------------------------------------------------------------------ 8. mg_compare_tri_sparse_host, mg_expand_tri_sparse

@pytest.mark.parametrize("engine", ["default", "sparse"])
@pytest.mark.parametrize("name", ["clades", "ragged_head", "families", "families_ragged"])
def test_tri_sparse_exceptions_and_their_expansion(eng, cases, tabs, name, engine, monkeypatch):
    _set_kernel(monkeypatch, engine)
    c, tab = cases[name], tabs[name]
    n, s = c["n"], c["s"]
    tab.invalidate()
    for rb, re in _ranges(name, c):
        lo, hi, pairs = _clamp(rb, re, n)
        want = helpers.edges_of_tri(c["numer"][lo:hi], c["denom"][lo:hi], rb, min(re, n))
        counted = engine == "sparse" and name == "families" and pairs >= 4000000
        if counted:
            eng.prof_enable(True)
            eng.prof_reset()
        cnt = C.c_uint64(0xDEAD)
        buf = np.empty(len(want) + 1, dtype=abi.EDGE_DTYPE)
        buf.view(np.uint32)[:] = SENTINEL
        rc = eng.lib.mg_compare_tri_sparse_host(eng.ctx, tab.handle, rb, re, buf.ctypes.data, len(want), C.byref(cnt))
        if counted:
            merged, filled = eng.prof_avg_ms("compare_merge")[1], eng.prof_avg_ms("compare_fill")[1]
            eng.prof_enable(False)
            assert merged >= 1 and filled == 0, (name, rb, re, merged, filled)                  # the lists, not the matrix
        assert rc == abi.MG_OK and cnt.value == len(want), (name, engine, rb, re, rc, cnt.value, len(want), eng.lib.mg_last_error(eng.ctx).decode())
        got = buf[:len(want)]
        assert np.all(buf[len(want):].view(np.uint32) == SENTINEL), "wrote past the exceptions"
        assert got.tobytes() == want.tobytes(), (name, engine, rb, re)                          # row and col: table indices
        key = got["row"].astype(np.int64) * n + got["col"]
        assert np.all(np.diff(key) > 0)                                                         # strictly ascending (row, col)
        dense = np.empty(pairs + 1, dtype=abi.COUNTS_DTYPE)
        dense.view(np.uint32)[:] = SENTINEL
        assert eng.lib.mg_expand_tri_sparse(got.ctypes.data if len(got) else None, len(got), c["nhash"].ctypes.data, s, rb, min(re, n),
                                            dense.ctypes.data) == abi.MG_OK
        assert np.all(dense[pairs:].view(np.uint32) == SENTINEL)
        assert dense[:pairs].tobytes() == helpers.expand_tri(want, c["nhash"], s, rb, re).tobytes()
        assert dense[:pairs].tobytes() == c["counts"][lo:hi].tobytes()
    if name == "families":                                                                      # shares a hash, numer 0: no exception
        row, col = c["where"]["behind"]
        got = eng.compare_tri_sparse(tab, row, row + 1)
        lo, hi, _ = _clamp(row, row + 1, n)
        assert got.tobytes() == helpers.edges_of_tri(c["numer"][lo:hi], c["denom"][lo:hi], row, row + 1).tobytes()
        assert not np.any(got["col"] == col)               # (the row is made of small values: it may have no exception at all)
    tab.invalidate()


def test_tri_sparse_capacity_protocol_and_expand_errors(eng, cases, tabs):
    c, tab = cases["clades"], tabs["clades"]
    rb, re = 31, 65
    lo, hi, pairs = _clamp(rb, re, c["n"])
    want = helpers.edges_of_tri(c["numer"][lo:hi], c["denom"][lo:hi], rb, re)
    n = C.c_uint64(0)

    def call(t, out, cap, cnt):
        return eng.lib.mg_compare_tri_sparse_host(eng.ctx, t, rb, re, out, cap, cnt)

    assert call(tab.handle, None, 0, C.byref(n)) == abi.MG_ERR_NOMEM and n.value == len(want) > 1
    buf = np.zeros(len(want) + 1, dtype=abi.EDGE_DTYPE)
    buf.view(np.uint32)[:] = SENTINEL
    n.value = 0
    assert call(tab.handle, buf.ctypes.data, len(want) - 1, C.byref(n)) == abi.MG_ERR_NOMEM and n.value == len(want)
    assert np.all(buf[len(want) - 1:].view(np.uint32) == SENTINEL)
    assert call(tab.handle, buf.ctypes.data, len(want), C.byref(n)) == abi.MG_OK and n.value == len(want)
    assert buf[:len(want)].tobytes() == want.tobytes() and np.all(buf[len(want):].view(np.uint32) == SENTINEL)
    assert call(None, buf.ctypes.data, len(want), C.byref(n)) == MG_ERR_INVALID
    assert call(tab.handle, buf.ctypes.data, len(want), None) == MG_ERR_INVALID
    assert call(tab.handle, None, len(want), C.byref(n)) == MG_ERR_INVALID
    # mg_expand_tri_sparse (host arithmetic) refuses what is no exception of the range
    dense = np.zeros(pairs, dtype=abi.COUNTS_DTYPE)
    nh = c["nhash"]

    def expand(edges, b=rb, e=re):
        edges = np.ascontiguousarray(edges)
        return eng.lib.mg_expand_tri_sparse(edges.ctypes.data, len(edges), nh.ctypes.data, c["s"], b, e, dense.ctypes.data)

    good = want.copy()
    assert expand(good) == abi.MG_OK and dense.tobytes() == c["counts"][lo:hi].tobytes()
    for field, row, col in (("below", rb - 1, 0), ("above", re, 0), ("diagonal", rb + 1, rb + 1), ("upper", rb + 1, rb + 2)):
        bad = good.copy()
        bad[len(bad) // 2]["row"], bad[len(bad) // 2]["col"] = row, col
        assert expand(bad) == MG_ERR_INVALID, field
    assert expand(good[:0], re, rb) == MG_ERR_INVALID                                          # row_begin > row_end
    assert expand(good) == abi.MG_OK and dense.tobytes() == c["counts"][lo:hi].tobytes()


# ------------------------------------------------------------------------------------------ 9. sharded forms with ranges

def _device_lists(*lists):
    """tests/test_gpu_parity.py's convention: the lists repeat device 0; MASHGPU_TEST_DEVICES=0,1,... adds distinct devices"""
    out = [list(l) for l in lists]
    extra = os.environ.get("MASHGPU_TEST_DEVICES")
    if extra:
        out.append([int(x) for x in extra.split(",")])
    return out


@pytest.mark.parametrize("weight", ["default", "0"])
@pytest.mark.parametrize("name", ["clades", "families"])
@pytest.mark.parametrize("devices", _device_lists([0, 0], [0, 0, 0]))
def test_sharded_tri_calls_with_ranges_equal_the_oracle(cases, host_fin, devices, name, weight, monkeypatch):
    """mg_compare_tri_*_sharded_host over several contexts with a caller's range: every context takes a block of the range's rows
    (from its own view of the table's first rows where the block is large enough), the blocks are joined in reference order"""
    if weight == "0":
        monkeypatch.setenv("MASHGPU_SHARD_ROW_WEIGHT", "0")
    c = cases[name]
    n = c["n"]
    max_d, max_p = FILTERS[name][0]
    host = host_fin(name, max_d, max_p)
    ranges = [(31, 65), (5, n + 1000), c["where"]["clades"][2]] if name == "clades" else [(1000, 3100), (0, 3200)]
    comm = abi.LocalComm(devices)
    try:
        d = comm.upload(c["table"], c["nhash"], c["lengths"])
        for rb, re in ranges:
            lo, hi, pairs = _clamp(rb, re, n)
            got = comm.tri(d, n, rb, re)
            assert got[:pairs].tobytes() == c["counts"][lo:hi].tobytes(), (rb, re)
            rec = comm.tri_pairs(d, n, K, KSPACE21, max_d, max_p, row_begin=rb, row_end=re)
            assert len(rec) == pairs
            _check_records_against_host(rec, host[lo:hi], max_d)
            _check_records_against_oracle(rec, c, lo, hi, max_d, max_p)
            want = _survivors(c, host, rb, re, max_d, max_p)
            res = comm.tri_results(d, n, K, KSPACE21, max_d, max_p, capacity=8, row_begin=rb, row_end=re)
            assert len(res) == len(want) > 8, (rb, re, len(res), len(want))
            assert res.tobytes() == want.tobytes(), (rb, re)
        # the defaults are the whole triangle
        if name == "clades":
            assert comm.tri_results(d, n, K, KSPACE21, max_d, max_p).tobytes() == _survivors(c, host, 0, n, max_d, max_p).tobytes()
            assert len(comm.tri_pairs(d, n, K, KSPACE21, max_d, max_p)) == tri_base(n)
        comm.free(d)
    finally:
        comm.close()
