"""Discovery leaves a row that has no partner to discover by a flag per row instead of a scan of the row's segment of both images
(SparseArgs::row_any: K5 sets it, the dense groups' encode writes it again for its rows, sp_discover_kernel reads it).

Every case is a triangle through mg_compare_tri_dev with the inverted-index engine forced, every pair compared with the oracle,
and run again with MASHGPU_DISCOVER_ROWFLAGS=0 (the scan): the two outputs must have the same bytes, and the MASHGPU_SPARSE_DBG
line of discovery must say which of the two ran.  Tables of a few hundred rows of s = 100 (a row stride of 104: K5's pieces of
32 positions end ragged), the smallest at which each path can go wrong:
  unrelated   every flag 0, no candidate;
  clades      clades of 20 and 40 near-copies among unrelated rows: dense groups are kept, the encode clears the flags K5 set
              inside them, and no candidate is left for the merge;
  mixed       two more clades with values planted across them (a row of a group keeps a non-empty run behind the clipping: the
              encode's flag 1), two rows outside every group that share values with clade rows and with each other (K5's flag
              stands), a row of 45 entries whose only non-empty run is its LAST entry and one whose only one is its FIRST;
  copies      the mixed table with exact copies of earlier rows (the DEDUP instantiation: copies bypass the flag, their
              representatives use it; such a table has no dense groups);
a row range that is not the whole table and a rect job (located runs of its own: the flags are not passed), one case under
MASHGPU_SPARSE_INDEX=verify (the flags are recomputed from the finished images behind the encode; a difference raises) and one
under =sort (the general sort writes no flags: the scan)."""
import re

import numpy as np
import pytest

from mash_amd import abi
from tests import helpers
from tests.helpers import tri_base

pytestmark = pytest.mark.gpu

K, KSPACE21 = 21, 4.0 ** 21
S = 100
TOP = 1 << 53
FLAGS, SCAN = "compare discover: rows without partners known by their flags", "compare discover: every row's segment scanned"


class _Maker:
    """rows of distinct values below 2^53; `fresh` never returns a value twice"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.used = set()
        self.rows = []
        self.clades = []

    def fresh(self, lo=1000, hi=TOP):
        while True:
            v = int(self.rng.integers(lo, hi))
            if v not in self.used:
                self.used.add(v)
                return v

    def single(self, count=S):
        self.rows.append(sorted(self.fresh() for _ in range(count)))
        return len(self.rows) - 1

    def clade(self, m):
        """m rows that keep nine tenths of a pool of S values of their own and add eight private ones"""
        pool = [self.fresh() for _ in range(S)]
        g0 = len(self.rows)
        for _ in range(m):
            v = [x for x in pool if self.rng.integers(10) != 0] + [self.fresh() for _ in range(8)]
            self.rows.append(sorted(v)[:S])
        self.clades.append((g0, len(self.rows)))


def _unrelated():
    m = _Maker(11)
    for _ in range(300):
        m.single()
    return m


def _clades():
    m = _Maker(12)
    for _ in range(40):
        m.single()
    m.clade(20)
    for k in range(30):
        m.single(int(m.rng.integers(1, S)) if k % 9 == 4 else S)           # (some of them short)
    m.clade(40)
    for _ in range(70):
        m.single()
    return m


def _mixed():
    m = _clades()
    m.clade(24)
    m.clade(33)
    A, B = m.clades[2], m.clades[3]
    m.cross = []
    for _ in range(5):                                      # a value planted in a row of each: in place of the row's largest
        v = m.fresh()
        a, b = int(m.rng.integers(*A)), int(m.rng.integers(*B))
        for r in (a, b):
            m.rows[r] = sorted(m.rows[r][:S - 1] + [v])
        m.cross.append((b, a))
    x, y = m.single(S - 3), m.single(S - 3)                 # outside every group: a value in common, and one of a clade row each
    both = m.fresh()
    m.rows[x] = sorted(m.rows[x] + [both, m.rows[m.clades[1][0] + 3][10]])
    m.rows[y] = sorted(m.rows[y] + [both, m.rows[m.clades[3][0] + 2][20]])
    m.outside = (x, y)
    early = 3
    big, small = m.rows[early][-1], m.rows[early][0]
    m.rows.append(sorted([m.fresh(1000, big) for _ in range(44)] + [big]))                   # its LAST entry only; 45 entries
    m.rows.append(sorted([small] + [m.fresh(small + 1, TOP) for _ in range(S - 1)]))          # its FIRST entry only
    m.last_only, m.first_only, m.early = len(m.rows) - 2, len(m.rows) - 1, early
    for _ in range(37):
        m.single()
    return m


def _copies():
    m = _mixed()
    for src in (5, m.outside[0], m.clades[1][0] + 1, m.last_only, 60):
        m.rows.append(list(m.rows[src]))
    m.rows.insert(100, list(m.rows[7]))                     # (a copy in the middle of the table as well)
    return m


def _shares(rows):
    """bool [n, n], lower triangle: the two rows have a value in common"""
    n = len(rows)
    M = np.zeros((n, n), dtype=bool)
    holders = {}
    for i, r in enumerate(rows):
        for v in r:
            holders.setdefault(v, []).append(i)
    for h in holders.values():
        if len(h) > 1:
            M[np.ix_(h, h)] = True
    return np.tril(M, -1)


def _arrays(rows, rng):
    table = np.full((len(rows), S), abi.HASH_PAD, dtype=np.uint64)
    nhash = np.zeros(len(rows), dtype=np.uint32)
    for i, r in enumerate(rows):
        table[i, :len(r)] = np.array(r, dtype=np.uint64)
        nhash[i] = len(r)
    return table, nhash, rng.integers(10 ** 4, 10 ** 8, len(rows)).astype(np.uint64)


@pytest.fixture(scope="module")
def cases(oracle):
    """table name -> the table, what it was made of, and the oracle's whole triangle: made once, on first use, read-only"""
    memo = {}
    make = {"unrelated": _unrelated, "clades": _clades, "mixed": _mixed, "copies": _copies}

    def get(name):
        if name not in memo:
            m = make[name]()
            table, nhash, lengths = _arrays(m.rows, np.random.default_rng(3))
            numer, denom, _, _ = oracle.triangle(table, nhash, lengths, 0, len(nhash), K, KSPACE21)
            counts = np.zeros(len(numer), dtype=abi.COUNTS_DTYPE)
            counts["numer"], counts["denom"] = numer, denom
            for a in (table, nhash, lengths, counts):
                a.flags.writeable = False
            memo[name] = {"made": m, "table": table, "nhash": nhash, "lengths": lengths, "counts": counts, "n": len(nhash), "shares": _shares(m.rows)}
        return memo[name]
    return get


@pytest.fixture(scope="module")
def eng():
    import torch
    torch.cuda.init()          # (torch ships its own HIP runtime: it initialises first, tests/test_gpu_parity.py)
    e = abi.MashGpu(0)
    e.set_option("MASHGPU_COSTS_FIXED", "1")
    yield e
    e.close()


@pytest.fixture
def sparse(monkeypatch):
    monkeypatch.setenv("MASHGPU_COMPARE_KERNEL", "sparse")
    monkeypatch.setenv("MASHGPU_COMPARE_JOIN", "0")          # (every candidate through discovery and the merge)
    monkeypatch.setenv("MASHGPU_SPARSE_DBG", "1")
    monkeypatch.delenv("MASHGPU_DISCOVER_ROWFLAGS", raising=False)
    monkeypatch.delenv("MASHGPU_SPARSE_INDEX", raising=False)


def _tri_dev(eng, tab, rb, re):
    """rows [rb, re) through mg_compare_tri_dev into a device buffer of this test's"""
    import torch
    pairs = tri_base(re) - tri_base(rb)
    buf = torch.full((max(pairs, 1) * 8,), 0xAB, dtype=torch.uint8, device="cuda")
    eng.compare_tri_dev(tab, rb, re, buf.data_ptr())
    torch.cuda.synchronize()
    return buf.cpu().numpy()[:pairs * 8].view(abi.COUNTS_DTYPE).copy()


def _check_tri(got, c, rb, re, what):
    want = c["counts"][tri_base(rb):tri_base(re)]
    if got.tobytes() != want.tobytes():
        bad = np.nonzero((got["numer"] != want["numer"]) | (got["denom"] != want["denom"]))[0]
        rows, cols = helpers.tri_rows_cols(rb, re)
        first = [(int(rows[i]), int(cols[i]), tuple(got[i]), tuple(want[i])) for i in bad[:5]]
        raise AssertionError(f"{what} rows [{rb}, {re}): {len(bad)} of {len(want)} pairs differ from the oracle; (row, col, got, want): {first}")


def _candidates(err):
    return [int(x) for x in re.findall(r"^compare merge: .+?, (\d+) candidates$", err, re.M)]


def _groups_kept(err):
    m = re.search(r"compare dense: \d+ chains of related rows, (\d+) groups kept \((\d+) rows", err)
    return (int(m.group(1)), int(m.group(2))) if m else (0, 0)


def _both_ways(eng, c, capfd, monkeypatch, rb, re, what, flags_line=FLAGS):
    """the job with the flags and with the scan, on a fresh table each (index and all): the oracle's pairs, the same bytes; returns
    what the first run said"""
    said = []
    outs = []
    for knob in (None, "0"):
        if knob is not None:
            monkeypatch.setenv("MASHGPU_DISCOVER_ROWFLAGS", knob)
        tab = eng.table_upload(c["table"], c["nhash"], c["lengths"])
        try:
            capfd.readouterr()
            outs.append(_tri_dev(eng, tab, rb, re))
        finally:
            tab.free()
        said.append(capfd.readouterr().err)
        assert "compare sparse: index of %d rows" % c["n"] in said[-1], said[-1][-2000:]       # the engine asked for is the one that ran
        ran = flags_line if knob is None else SCAN
        assert ran in said[-1] and (SCAN if ran == FLAGS else FLAGS) not in said[-1], said[-1][-2000:]
        _check_tri(outs[-1], c, rb, re, (what, "flags" if knob is None else "scan"))
    monkeypatch.delenv("MASHGPU_DISCOVER_ROWFLAGS")
    assert outs[0].tobytes() == outs[1].tobytes(), what
    assert _candidates(said[0]) == _candidates(said[1]), what
    return said[0]


def test_unrelated_rows_have_no_flag_and_no_candidate(eng, cases, sparse, capfd, monkeypatch):
    c = cases("unrelated")
    assert not c["shares"].any()
    err = _both_ways(eng, c, capfd, monkeypatch, 0, c["n"], "unrelated")
    assert "index by tiles" in err and _candidates(err) == [], err[-2000:]
    assert int(c["counts"]["numer"].max()) == 0


def _outside_groups(c):
    """the sharing pairs that do not lie inside one clade"""
    inside = np.zeros_like(c["shares"])
    for g0, g1 in c["made"].clades:
        inside[g0:g1, g0:g1] = True
    return c["shares"] & ~inside


def test_clades_kept_as_groups_leave_nothing_to_discover(eng, cases, sparse, capfd, monkeypatch):
    c = cases("clades")
    m = c["made"]
    assert not _outside_groups(c).any() and c["shares"].sum() >= 20 * 19 // 2 + 40 * 39 // 2 - 5
    err = _both_ways(eng, c, capfd, monkeypatch, 0, c["n"], "clades")
    assert "index by tiles" in err and _groups_kept(err) == (2, 60), err[-2000:]
    assert _candidates(err) == [], err[-2000:]             # every run inside a group clipped to nothing: the encode cleared the flags


def test_mixed_table_cross_pairs_and_edge_entries(eng, cases, sparse, capfd, monkeypatch):
    c = cases("mixed")
    m = c["made"]
    outside = _outside_groups(c)
    for b, a in m.cross:                                    # planted across two groups
        assert outside[max(a, b), min(a, b)]
    x, y = m.outside
    assert outside[y, x] and outside[x].sum() >= 1 and outside[y].sum() >= 2
    assert outside[m.last_only].sum() == 1 and outside[m.last_only, m.early] and len(m.rows[m.last_only]) == 45
    assert outside[m.first_only].sum() == 1 and outside[m.first_only, m.early]
    assert m.rows[m.last_only][-1] == m.rows[m.early][-1] and m.rows[m.first_only][0] == m.rows[m.early][0]
    err = _both_ways(eng, c, capfd, monkeypatch, 0, c["n"], "mixed")
    assert "index by tiles" in err and _groups_kept(err) == (4, 117), err[-2000:]
    # every pair that shares a value across the groups' borders is a candidate (pairs inside a group may be discovered as well:
    # both engines then write the same counts)
    cand = _candidates(err)
    assert len(cand) == 1 and int(outside.sum()) <= cand[0] <= int(c["shares"].sum()), err[-2000:]
    # (the value the two rows' last entries share lies behind the s-th element of their union: a candidate whose count is 0;
    #  the shared first entry counts)
    assert int(c["counts"]["numer"][tri_base(m.last_only) + m.early]) == 0 and int(c["counts"]["numer"][tri_base(m.first_only) + m.early]) == 1


def test_copies_bypass_the_flag_and_their_representatives_use_it(eng, cases, sparse, capfd, monkeypatch):
    c = cases("copies")
    err = _both_ways(eng, c, capfd, monkeypatch, 0, c["n"], "copies")
    assert "(6 copies of earlier rows)" in err and "index by tiles" in err, err[-2000:]
    assert _groups_kept(err) == (0, 0), err[-2000:]


def test_a_row_range_that_is_not_the_whole_table(eng, cases, sparse, capfd, monkeypatch):
    c = cases("mixed")
    m = c["made"]
    rb, re_ = m.clades[1][0] + 7, m.first_only + 1            # from inside a clade to the row whose first entry alone has a run
    assert 0 < rb and re_ < c["n"] and _outside_groups(c)[rb:re_].any()
    _both_ways(eng, c, capfd, monkeypatch, rb, re_, "mixed, a range")


def test_rect_job_locates_its_own_runs(eng, oracle, cases, sparse, capfd, monkeypatch):
    """the queries' runs are located per call: nobody flagged them, the scan stays -- with the knob either way"""
    c = cases("mixed")
    m = c["made"]
    qrows = [m.rows[r] for r in (0, m.clades[0][0] + 2, m.outside[1], m.last_only, m.first_only)] + [sorted(m.fresh() for _ in range(S))]
    qt, qn, ql = _arrays(qrows, np.random.default_rng(4))
    numer, denom, _, _ = helpers.rect_oracle(oracle, c["table"], c["nhash"], c["lengths"], qt, qn, ql, K, KSPACE21)
    assert (numer[:5].max(axis=1) >= 1).all() and int(numer[5].max()) == 0
    outs = []
    for knob in (None, "0"):
        if knob is not None:
            monkeypatch.setenv("MASHGPU_DISCOVER_ROWFLAGS", knob)
        ref, qry = eng.table_upload(c["table"], c["nhash"], c["lengths"]), eng.table_upload(qt, qn, ql)
        try:
            capfd.readouterr()
            got = eng.compare_rect_host(ref, qry)
        finally:
            ref.free()
            qry.free()
        err = capfd.readouterr().err
        assert SCAN in err and FLAGS not in err, err[-2000:]
        assert np.array_equal(got["numer"], numer) and np.array_equal(got["denom"], denom), knob
        outs.append(got.tobytes())
    assert outs[0] == outs[1]


def test_verify_recomputes_the_flags_behind_the_encode(eng, cases, sparse, capfd, monkeypatch):
    """MASHGPU_SPARSE_INDEX=verify: a flag that differs from what the finished images say fails the call"""
    c = cases("mixed")
    monkeypatch.setenv("MASHGPU_SPARSE_INDEX", "verify")
    err = _both_ways(eng, c, capfd, monkeypatch, 0, c["n"], "mixed, verify")
    assert "index by tiles" in err and _groups_kept(err) == (4, 117), err[-2000:]


def test_the_general_sort_writes_no_flags(eng, cases, sparse, capfd, monkeypatch):
    c = cases("mixed")
    monkeypatch.setenv("MASHGPU_SPARSE_INDEX", "sort")
    err = _both_ways(eng, c, capfd, monkeypatch, 0, c["n"], "mixed, sort", flags_line=SCAN)
    assert "index by tiles" not in err and _groups_kept(err)[0] >= 1, err[-2000:]
