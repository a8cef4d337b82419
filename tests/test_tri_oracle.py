"""The judge of tests/test_tri_gpu.py, checked on the CPU: the flat order of oracle.triangle against oracle.compare pair by
pair, helpers.tri_slice / tri_rows_cols against a double loop, helpers.expand_tri (the rule of mg_compare_tri_sparse_host,
include/mashgpu.h) against the oracle's dense counts, whole and in ranges.  Then the conditions the GPU tests' tables must
meet, on the oracle's output alone."""
import numpy as np
import pytest

from tests import helpers

K, KSPACE21 = 21, 4.0 ** 21


@pytest.fixture(scope="module")
def tri_cases(oracle):
    """name -> (case, the oracle's whole triangle); computed once, read-only"""
    out = {}
    for name in ("families", "families_ragged", "clades", "species"):
        case = getattr(helpers, "tri_case_" + name)()
        flat = helpers.tri_case_oracle(oracle, case, K, KSPACE21)
        for a in flat:
            a.flags.writeable = False
        out[name] = (case, flat)
    return out


def test_tri_slice_and_rows_cols_against_a_double_loop():
    n = 12
    pairs = [(i, j) for i in range(n) for j in range(i)]                    # reference order: row i against rows j < i
    flat = np.arange(len(pairs), dtype=np.int64)
    for rb in range(n + 1):
        for re in range(rb, n + 1):
            want = [(p, ij) for p, ij in enumerate(pairs) if rb <= ij[0] < re]
            assert list(helpers.tri_slice(flat, rb, re)) == [p for p, _ in want], (rb, re)
            rows, cols = helpers.tri_rows_cols(rb, re)
            assert list(zip(rows.tolist(), cols.tolist())) == [ij for _, ij in want], (rb, re)
    assert helpers.tri_base(0) == helpers.tri_base(1) == 0 and helpers.tri_base(5) == 10
    assert len(helpers.tri_slice(flat, 0, 1)) == 0 and len(helpers.tri_slice(flat, 7, 3)) == 0       # row 0 has no pair


@pytest.mark.parametrize("name", ["families", "families_ragged", "clades", "species"])
def test_tri_tables_meet_their_conditions(tri_cases, name):
    case, (numer, denom, dist, pval) = tri_cases[name]
    helpers.check_tri_case_conditions(name, case, numer, denom, dist, pval)


@pytest.mark.parametrize("name", ["clades", "families_ragged"])
def test_expand_tri_of_the_exceptions_is_the_oracles_counts(oracle, tri_cases, name):
    case, (numer, denom, _, _) = tri_cases[name]
    n, s = case["n"], case["s"]
    for rb, re in ((0, n), (3, 8), (0, 1), (0, 2), (n, n), (n - 40, n + 7)):
        nn, dd, _, _ = oracle.triangle(case["table"], case["nhash"], case["lengths"], rb, re, K, KSPACE21)
        assert np.array_equal(nn, helpers.tri_slice(numer, rb, min(re, n))) and np.array_equal(dd, helpers.tri_slice(denom, rb, min(re, n)))
        edges = helpers.edges_of_tri(nn, dd, rb, min(re, n))
        assert np.all(edges["col"] < edges["row"]) and np.all(edges["numer"] >= 1) and len(edges) == int((nn >= 1).sum())
        key = edges["row"].astype(np.int64) * n + edges["col"]
        assert np.all(np.diff(key) > 0)                                                # reference order is ascending (row, col)
        got = helpers.expand_tri(edges, case["nhash"], s, rb, re)
        assert np.array_equal(got["numer"], nn) and np.array_equal(got["denom"], dd), (name, rb, re)
        if (rb, re) == (0, n):
            assert 0 < len(edges) < len(nn)
        if (rb, re) in ((0, 1), (n, n)):
            assert len(got) == 0 and len(edges) == 0
    # an exception is what it says: one dropped, and that pair falls back to the rule
    rb = n - 40
    nn, dd = helpers.tri_slice(numer, rb, n), helpers.tri_slice(denom, rb, n)
    edges = helpers.edges_of_tri(nn, dd, rb, n)
    assert len(edges) >= 2
    less = helpers.expand_tri(edges[1:], case["nhash"], s, rb, n)
    assert int((less["numer"] != nn).sum()) == 1


def test_oracle_flat_order_against_single_compares(oracle, tri_cases):
    case, (numer, denom, dist, pval) = tri_cases["families_ragged"]
    t, nh, ln, s = case["table"], case["nhash"], case["lengths"], case["s"]
    e0, e1 = case["where"]["empty"]
    pairs = [(1, 0), (2, 0), (2, 1), (3199, 0), (3199, 3198), (2000, 1999), (3100, 7), (e1, e0), (case["where"]["one_hash"], 3),
             (1234, case["where"]["one_hash"]), (case["where"]["one_short"], 100), (50, 49), (3001, 11), (1001, 17)]
    rng = np.random.default_rng(12)
    pairs += [(int(i), int(rng.integers(0, i))) for i in rng.integers(1, 3200, 40)]
    assert nh[50] < s                                                                  # (a short row among them)
    for i, j in pairs:
        o = oracle.compare(t[j, : nh[j]], t[i, : nh[i]], int(ln[j]), int(ln[i]), s, K, KSPACE21)
        at = helpers.tri_base(i) + j
        assert (int(numer[at]), int(denom[at])) == (o.numer, o.denom), (i, j)
        assert dist[at] == o.distance and pval[at] == o.p_value, (i, j)
    at = helpers.tri_base(e1) + e0
    assert (int(numer[at]), int(denom[at])) == (0, 0)                                  # empty against empty
