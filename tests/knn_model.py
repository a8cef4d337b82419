"""The definition of `mash triangle -N` / mg_compare_tri_topk_host in pure Python (exact integers), for the tests.

For row i of a table of n sketches the neighbours are all j != i; the record of (i, j) is the record of the unordered pair
(the `mash triangle -E` line of (max(i, j), min(i, j))), eligible iff that pair passes the filters; the order is
tests/topk_model.py's on the exact fraction with the NEIGHBOUR index as the second key, one order across both sides of the
diagonal; the result is the first min(k, eligible) neighbours of every row, rows ascending.

knn_of_pairs works on the packed triangle (pair (i, j), j < i, at i (i - 1) / 2 + j); knn_of_stdout applies the same to a
recorded `mash triangle -E` stdout: a line gives both its rows an entry, a filter's survivors are exactly the lines present."""
import functools

import numpy as np

from tests import topk_model as tm


def tri_index(i, j):
    """place of the unordered pair {i, j}, i != j, in the packed triangle"""
    hi, lo = (i, j) if i > j else (j, i)
    return hi * (hi - 1) // 2 + lo


def symmetrise(values, n, fill=0):
    """packed triangle -> [n][n], the diagonal `fill`"""
    values = np.asarray(values)
    full = np.full((n, n), fill, dtype=values.dtype)
    i, j = np.tril_indices(n, -1)                              # row major, j < i: the packed order
    full[i, j] = values
    full[j, i] = values
    return full


def rank_rows(numer, denom, passed, n):
    """packed triangles -> (order [n][n - 1 and more], count [n]): row i's neighbours best first are order[i][:count[i]].
    Rows are ranked by topk_model.rank_row_fast.  Where every denominator is below 2^26 -- every table of the tests -- the whole
    table is ranked at once instead, exactly: a float64 quotient of two such integers is correctly rounded, so equal fractions
    give the same double, and two different fractions lie at least 2^-52 apart in relative terms, more than one rounding; a stable
    sort of the quotients, descending, keeps equal fractions in ascending neighbour order.  tests/test_knn_model.py holds the two
    against each other."""
    nm, dn = symmetrise(np.asarray(numer, dtype=np.uint64), n), symmetrise(np.asarray(denom, dtype=np.uint64), n)
    ok = symmetrise(np.ones(n * (n - 1) // 2, dtype=bool) if passed is None else np.asarray(passed, dtype=bool), n, False)
    count = ok.sum(axis=1)                                     # (the diagonal is False: self is dropped)
    if n and int(dn.max()) < (1 << 26):
        q = nm.astype(np.float64) / np.maximum(dn, 1).astype(np.float64)      # (0/0 ranks as 0/1)
        q[~ok] = -1.0
        return np.argsort(-q, axis=1, kind="stable"), count
    return [tm.rank_row_fast(nm[i], dn[i], ok[i], n) for i in range(n)], count


def knn_of_pairs(numer, denom, passed, n, k):
    """numer, denom, passed (None: every pair): packed triangles of n rows -> per row the list of neighbour indices, best first"""
    order, count = rank_rows(numer, denom, passed, n)
    return [[int(j) for j in order[i][:min(k, int(count[i]))]] for i in range(n)]


def entries_of_stdout(stdout, names):
    """a recorded `triangle -E` stdout -> per row of `names` the list of (numer, denom, neighbour index, line fields behind the names)"""
    at = {nm: i for i, nm in enumerate(names)}
    assert len(at) == len(names), "names must be unique"
    rows = [[] for _ in names]
    for ln in stdout.splitlines():
        f = ln.split("\t")
        i, j = at[f[0]], at[f[1]]
        x, y = f[4].split("/")
        rows[i].append((int(x), int(y), j, f[2:]))
        rows[j].append((int(x), int(y), i, f[2:]))
    return rows


def ranked_entries(stdout, names):
    rows = entries_of_stdout(stdout, names)
    for r in rows:
        r.sort(key=functools.cmp_to_key(lambda a, b: tm._cmp(a[:3], b[:3])))
    return rows


def knn_of_stdout(stdout, names, k):
    """what `mash triangle -N k` prints where `mash triangle -E` (same options) printed `stdout`; names: the sketches in input order"""
    out = []
    for i, r in enumerate(ranked_entries(stdout, names)):
        for e in r[:k]:
            out.append("\t".join([names[i], names[e[2]], *e[3]]) + "\n")
    return "".join(out)


def same_fraction(a, b):
    return a[0] * (b[1] or 1) == b[0] * (a[1] or 1)


def has_tie_across_cut(stdout, names, k):
    """some row's k-th and (k+1)-th ranked neighbours carry equal fractions"""
    return any(len(r) > k and same_fraction(r[k - 1], r[k]) for r in ranked_entries(stdout, names))


def has_tie_across_diagonal(stdout, names):
    """some row i has two neighbours of equal fraction, one below i and one above"""
    for i, r in enumerate(ranked_entries(stdout, names)):
        for a, b in zip(r, r[1:]):
            if same_fraction(a, b) and (a[2] < i) != (b[2] < i):
                return True
    return False
