"""The row blocks behind the matrix outputs (host_compare.cpp: matrix_blocks), cut small by MASHGPU_OUT_BLOCK_PAIRS.

mg_compare_{tri,rect}_host, *_pairs_host, *_filter_host and *_results_host walk their range in blocks of whole rows of up to 2^26 ..
2^30 pairs, so on tables of test size the bookkeeping between blocks -- the pairs before a block, the survivors so far, the room left
in the caller's buffer, where the next block writes -- never runs.  The knob lowers the block size (a block always takes its first
row): 1 pair gives one row per block, a size that no number of rows adds up to gives ragged blocks, 2^30 gives one block.  With
MASHGPU_RESULTS_MATRIX=1 the thresholded outputs take the blocks too.

The judge is the oracle (tri_case_oracle / rect_case_oracle), as in test_tri_gpu.py and test_rect_gpu.py; that the output does
not depend on the block size is asserted on top of that, never in its place."""
import ctypes as C

import numpy as np
import pytest

from mash_amd import abi
from tests import helpers
from tests.helpers import _check_records_against_oracle, _oracle_pass, _set_kernel

pytestmark = pytest.mark.gpu

K, KSPACE21 = 21, 4.0 ** 21
# -d at a threshold, -d plus -v.  In rect_case_clean every pair that shares a hash is a close relative whose p-value underflows to
# 0: no -v removes any of them.  So the ragged rect case runs beside it, where -v 1e-100 removes a tenth of what -d 0.1 passes (in
# the triangle -v 1e-150 removes a third): a wrong p-value filter across blocks shows in both forms.
FILTERS = {"tri": ((0.05, -1.0), (0.05, 1e-150)), "rect": ((0.05, -1.0), (0.05, 1e-30)), "rect_ragged": ((0.1, -1.0), (0.1, 1e-100))}
RECT_BLOCKS = (1, 2 * 1200 + 1, 1 << 30)
BLOCKS = {"tri": (1, 4097, 1 << 30), "rect": RECT_BLOCKS, "rect_ragged": RECT_BLOCKS}       # the middle one: no multiple of any row length
QUERIES = {"rect": (5, 80), "rect_ragged": (3, 37)}    # proper ranges of the rect cases' 87 and 40 queries
FORMS = ["tri", "rect", "rect_ragged"]


class Job:
    """One range of one case: the oracle's arrays of the range, flat in reference order, and the library's calls over it"""

    def __init__(self, form, oracle):
        self.form, self.eng, self.tabs = form.split("_")[0], None, ()
        if form == "tri":
            c = helpers.tri_case_head(helpers.tri_case_families(), 300)
            flat = helpers.tri_case_oracle(oracle, c, K, KSPACE21)
            self.first, self.last = 0, c["n"]
            self.rows, self.cols = helpers.tri_rows_cols(0, c["n"])
            self.row_pairs = np.arange(c["n"])                             # row i: i pairs
            self.tables = ((c["table"], c["nhash"], c["lengths"]),)
        else:
            c = helpers.rect_case_clean() if form == "rect" else helpers.rect_case_ragged()
            qb, qe = QUERIES[form]
            nq, nref = len(c["qn"]), len(c["rn"])
            assert 0 < qb < qe < nq and RECT_BLOCKS[1] == 2 * nref + 1
            flat = [a[qb:qe].reshape(-1) for a in helpers.rect_case_oracle(oracle, c, K, KSPACE21)]
            self.first, self.last = qb, qe
            self.rows, self.cols = np.repeat(np.arange(qb, qe), nref), np.tile(np.arange(nref), qe - qb)
            self.row_pairs = np.full(qe - qb, nref)
            self.tables = ((c["rt"], c["rn"], c["rl"]), (c["qt"], c["qn"], c["ql"]))
        self.c = dict(zip(("numer", "denom", "dist", "pval"), flat))
        assert len(self.rows) == len(self.c["numer"]) == int(self.row_pairs.sum())
        if form == "tri":
            assert len(self.rows) == 44850
        self.counts = np.zeros(len(self.rows), dtype=abi.COUNTS_DTYPE)
        self.counts["numer"], self.counts["denom"] = self.c["numer"], self.c["denom"]

    def upload(self, eng):
        self.eng, self.tabs = eng, tuple(eng.table_upload(*t) for t in self.tables)

    def free(self):
        for t in self.tabs:
            t.free()

    def _call(self, name, *args):
        fn = getattr(self.eng.lib, f"mg_compare_{self.form}_{name}")
        return fn(self.eng.ctx, *[t.handle for t in self.tabs], self.first, self.last, *args)

    def counts_host(self):
        out = np.zeros(len(self.rows) + 1, dtype=abi.COUNTS_DTYPE)
        out.view(np.uint8)[:] = 0xA5
        assert self._call("host", out.ctypes.data) == abi.MG_OK, self.eng.lib.mg_last_error(self.eng.ctx).decode()
        assert np.all(out[-1:].view(np.uint8) == 0xA5), "wrote past the range"
        return out[:-1]

    def pairs_host(self, max_d, max_p):
        out = np.zeros(len(self.rows) + 1, dtype=abi.PAIR_DTYPE)
        out.view(np.uint8)[:] = 0xA5
        assert self._call("pairs_host", K, KSPACE21, max_d, max_p, out.ctypes.data) == abi.MG_OK, self.eng.lib.mg_last_error(self.eng.ctx).decode()
        assert np.all(out[-1:].view(np.uint8) == 0xA5), "wrote past the range"
        return out[:-1]

    def listed(self, which, max_d, max_p, capacity):
        """*_filter_host / *_results_host into a buffer of `capacity` records with a guard record behind (capacity None: NULL and
        0): (rc, count, the records if rc is MG_OK)"""
        dtype = abi.EDGE_DTYPE if which == "filter" else abi.RESULT_DTYPE
        n = C.c_uint64(0xDEAD)
        buf = None if capacity is None else np.empty(capacity + 1, dtype=dtype)
        if buf is not None:
            buf.view(np.uint8)[:] = 0xA5
        tail = (None if buf is None else buf.ctypes.data, capacity or 0, C.byref(n))
        rc = self._call("filter_host", K, max_d, *tail) if which == "filter" else self._call("results_host", K, KSPACE21, max_d, max_p, *tail)
        if buf is None:
            return rc, n.value, None
        assert np.all(buf[capacity:].view(np.uint8) == 0xA5), "wrote past the buffer"
        if rc != abi.MG_OK:
            return rc, n.value, None
        assert np.all(buf[n.value:].view(np.uint8) == 0xA5), "wrote past the survivors"
        return rc, n.value, buf[:n.value]

    def passing(self, which, max_d, max_p):
        """where the oracle's survivors are in the range: *_filter_host knows the distance alone"""
        return np.nonzero(self.c["dist"] <= max_d if which == "filter" else _oracle_pass(self.c, max_d, max_p))[0]

    def check_listed(self, which, got, max_d, max_p):
        """a complete list of survivors against the oracle: who, in which order, the integers and the distance exactly, the
        p-value at the oracle's own accuracy"""
        at = self.passing(which, max_d, max_p)
        assert len(got) == len(at)
        assert np.array_equal(got["row"], self.rows[at]) and np.array_equal(got["col"], self.cols[at])
        if which == "filter":
            want = np.zeros(len(at), dtype=abi.EDGE_DTYPE)
            want["row"], want["col"], want["numer"], want["denom"] = self.rows[at], self.cols[at], self.c["numer"][at], self.c["denom"][at]
            assert got.tobytes() == want.tobytes()
            return
        rec = np.zeros(len(at), dtype=abi.PAIR_DTYPE)
        for f in ("numer", "denom", "distance", "p_value"):
            rec[f] = got[f]
        rec["pass"] = 1
        _check_records_against_oracle(rec, {f: a[at] for f, a in self.c.items()}, 0, len(at), max_d, max_p)


def block_of_row(row_pairs, max_pairs):
    """host_compare.cpp's row_blocks: whole rows while they fit max_pairs pairs, a block always takes its first row"""
    out, blk, pairs = [], 0, 0
    for add in row_pairs:
        if pairs and pairs + add > max_pairs:
            blk, pairs = blk + 1, 0
        pairs += int(add)
        out.append(blk)
    return np.array(out)


@pytest.fixture(scope="module")
def eng():
    import torch
    torch.cuda.init()          # (torch ships its own HIP runtime: it initialises first, tests/test_gpu_parity.py)
    e = abi.MashGpu(0)
    e.set_option("MASHGPU_COSTS_FIXED", "1")
    yield e
    e.close()


@pytest.fixture(scope="module")
def jobs(request, oracle):
    out = {form: Job(form, oracle) for form in FORMS}
    for form, job in out.items():
        # Before the GPU is touched: at the middle block size the survivors of every filter lie in three blocks or more (and the
        # blocks are ragged: more than one row in some, never a whole number of rows' worth) -- else the tests below prove nothing
        blocks = block_of_row(job.row_pairs, BLOCKS[form][1])
        assert blocks[-1] >= 8 and np.bincount(blocks).max() >= 2
        for max_d, max_p in FILTERS[form]:
            for which in ("filter", "results"):
                at = job.passing(which, max_d, max_p)
                assert 8 <= len(at) < len(job.rows) // 2
                assert len(np.unique(blocks[job.rows[at] - job.first])) >= 3, (form, which, max_d, max_p)
    for form in ("tri", "rect_ragged"):                                                   # -v removes some of what -d passes, not all
        only_d, both = (len(out[form].passing("results", *f)) for f in FILTERS[form])
        assert 0.5 * only_d < both < 0.95 * only_d, (form, only_d, both)
    eng = request.getfixturevalue("eng")
    for job in out.values():
        job.upload(eng)
    yield out
    for job in out.values():
        job.free()


def _matrix_route(monkeypatch, block_pairs=None):
    _set_kernel(monkeypatch, "default")
    monkeypatch.setenv("MASHGPU_RESULTS_MATRIX", "1")
    if block_pairs is None:
        monkeypatch.delenv("MASHGPU_OUT_BLOCK_PAIRS", raising=False)
    else:
        monkeypatch.setenv("MASHGPU_OUT_BLOCK_PAIRS", str(block_pairs))


@pytest.mark.parametrize("form", FORMS)
def test_counts_and_pairs_do_not_depend_on_the_blocks(jobs, form, monkeypatch):
    job = jobs[form]
    _matrix_route(monkeypatch)
    counts = job.counts_host()
    assert counts.tobytes() == job.counts.tobytes()
    pairs = {f: job.pairs_host(*f) for f in FILTERS[form]}
    for (max_d, max_p), rec in pairs.items():
        _check_records_against_oracle(rec, job.c, 0, len(rec), max_d, max_p)
    launches = {}
    for block_pairs in BLOCKS[form]:
        _matrix_route(monkeypatch, block_pairs)
        job.eng.prof_enable(True)
        job.eng.prof_reset()
        got = job.counts_host()
        launches[block_pairs] = job.eng.prof_avg_ms("compare")[1]
        job.eng.prof_enable(False)
        assert got.tobytes() == counts.tobytes(), block_pairs
        for (max_d, max_p), rec in pairs.items():
            got = job.pairs_host(max_d, max_p)
            _check_records_against_oracle(got, job.c, 0, len(got), max_d, max_p)
            assert got.tobytes() == rec.tobytes(), (block_pairs, max_d, max_p)
    # the knob really cut the range: a block is a compare launch at least (one per density class of its rows)
    rows = len(job.row_pairs) - (form == "tri")                                          # (row 0 goes with row 1)
    assert launches[1] >= rows and launches[1] > launches[1 << 30] >= 1, launches


@pytest.mark.parametrize("which", ["filter", "results"])
@pytest.mark.parametrize("form", FORMS)
def test_survivors_do_not_depend_on_the_blocks(jobs, form, which, monkeypatch):
    job = jobs[form]
    for max_d, max_p in FILTERS[form] if which == "results" else FILTERS[form][:1]:
        n_want = len(job.passing(which, max_d, max_p))
        _matrix_route(monkeypatch)
        rc, count, base = job.listed(which, max_d, max_p, n_want)
        assert (rc, count) == (abi.MG_OK, n_want), job.eng.lib.mg_last_error(job.eng.ctx).decode()
        job.check_listed(which, base, max_d, max_p)
        for block_pairs in BLOCKS[form]:
            _matrix_route(monkeypatch, block_pairs)
            rc, count, got = job.listed(which, max_d, max_p, n_want)
            assert (rc, count) == (abi.MG_OK, n_want), (block_pairs, job.eng.lib.mg_last_error(job.eng.ctx).decode())
            job.check_listed(which, got, max_d, max_p)
            assert got.tobytes() == base.tobytes(), (block_pairs, max_d, max_p)


@pytest.mark.parametrize("which", ["filter", "results"])
@pytest.mark.parametrize("form", FORMS)
def test_capacity_protocol_across_blocks(jobs, form, which, monkeypatch):
    """A buffer that is short in the last block, one of a single record -- short in the first block with survivors at the middle
    block size, where that block holds several; with one row per block in the first or the second --, and none at all:
    MG_ERR_NOMEM with the true count, nothing written behind the buffer (Job.listed asserts the guard), and the retry at full
    capacity gives the same bytes"""
    job = jobs[form]
    max_d, max_p = FILTERS[form][-1] if which == "results" else FILTERS[form][0]
    at = job.passing(which, max_d, max_p)
    _matrix_route(monkeypatch)
    rc, count, base = job.listed(which, max_d, max_p, len(at))
    assert (rc, count) == (abi.MG_OK, len(at))
    job.check_listed(which, base, max_d, max_p)
    for block_pairs in BLOCKS[form][:2]:
        blocks = block_of_row(job.row_pairs, block_pairs)[job.rows[at] - job.first]          # the block of every survivor
        assert (blocks == blocks[0]).sum() < len(at) - 1 and blocks[-1] != blocks[0]          # capacity n - 1 holds the first block's
        if block_pairs != 1:
            assert (blocks == blocks[0]).sum() >= 2                                           # capacity 1 does not
        _matrix_route(monkeypatch, block_pairs)
        for capacity in (len(at) - 1, 1, None):
            rc, count, _ = job.listed(which, max_d, max_p, capacity)
            assert (rc, count) == (abi.MG_ERR_NOMEM, len(at)), (block_pairs, capacity)
        rc, count, got = job.listed(which, max_d, max_p, len(at))
        assert (rc, count) == (abi.MG_OK, len(at)) and got.tobytes() == base.tobytes(), block_pairs
