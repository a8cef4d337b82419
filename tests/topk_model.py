"""The definition of `mash dist -N` / mg_compare_rect_topk_host in pure Python (exact integers), for the tests.

For a query, the eligible references are those whose pair passes the filters.  Pair a ranks before pair b iff
numer_a * denom_b > numer_b * denom_a; a pair of two empty sketches (0/0) is compared as 0/1, so numer == 0 ranks as zero
whatever its denom; equal fractions by ascending reference index.  The result is the first min(k, eligible) pairs.

rank_row / topk work on arrays of {numer, denom, pass}; topk_of_stdout applies the same to a recorded `mash dist` stdout
through its column 5 ("numer/denom"): the reference prints a query's lines in reference order, so the line number inside a
query's run IS the reference order, and a filter's survivors are exactly the lines present."""
import functools


def _cmp(a, b):
    """a, b: (numer, denom, index)"""
    l = int(a[0]) * (int(b[1]) or 1)
    r = int(b[0]) * (int(a[1]) or 1)
    if l != r:
        return -1 if l > r else 1
    return -1 if a[2] < b[2] else (1 if a[2] > b[2] else 0)


def rank_row(numer, denom, passed, k):
    """reference indices of one query's answer, best first"""
    items = [(int(numer[r]), int(denom[r]), r) for r in range(len(numer)) if passed is None or passed[r]]
    items.sort(key=functools.cmp_to_key(_cmp))
    return [it[2] for it in items[:k]]


def topk(numer, denom, passed, k):
    """numer, denom, passed: [nq][nref] -> per query the list of reference indices"""
    return [rank_row(numer[q], denom[q], None if passed is None else passed[q], k) for q in range(len(numer))]


def query_runs(stdout):
    """a recorded `mash dist` stdout -> [(query name, [line, ...])] in order of appearance.  Lines of one query are contiguous
    (the output is query major); neighbouring queries must not share a name."""
    runs = []
    for ln in stdout.splitlines(keepends=True):
        q = ln.split("\t")[1]
        if not runs or runs[-1][0] != q:
            runs.append((q, []))
        runs[-1][1].append(ln)
    return runs


def fraction_of_line(ln):
    x, y = ln.rstrip("\n").split("\t")[4].split("/")
    return int(x), int(y)


def topk_of_stdout(stdout, k):
    """what `mash dist -N k` prints where `mash dist` (same options) printed `stdout`"""
    out = []
    for _, lines in query_runs(stdout):
        fr = [fraction_of_line(ln) for ln in lines]
        for r in rank_row([f[0] for f in fr], [f[1] for f in fr], None, k):
            out.append(lines[r])
    return "".join(out)


def has_tie_across_cut(stdout, k):
    """some query's k-th and (k+1)-th ranked lines carry equal fractions"""
    for _, lines in query_runs(stdout):
        fr = [fraction_of_line(ln) for ln in lines]
        order = rank_row([f[0] for f in fr], [f[1] for f in fr], None, k + 1)
        if len(order) > k:
            a, b = fr[order[k - 1]], fr[order[k]]
            if a[0] * (b[1] or 1) == b[0] * (a[1] or 1):
                return True
    return False


def rank_row_fast(numer, denom, passed, k):
    """rank_row for long rows (numpy arrays): the exact ranking runs on a superset of the answer chosen by a float64 quotient.
    A float64 quotient of two integers below 2^32 is within a relative 2^-52 of the fraction, so a pair whose quotient lies
    below (1 - 1e-9) of the k-th largest quotient ranks after k pairs for certain and cannot be part of the answer.  Where the
    k-th largest quotient is 0 the row is completed by numer == 0 pairs, which tie in index order: the first k of them can be."""
    import numpy as np
    numer = np.asarray(numer, dtype=np.uint64)
    denom = np.asarray(denom, dtype=np.uint64)
    idx = np.arange(len(numer)) if passed is None else np.nonzero(np.asarray(passed))[0]
    if len(idx) > max(4 * k, 64):
        key = numer[idx].astype(np.float64) / np.maximum(denom[idx], 1).astype(np.float64)
        kth = np.partition(key, len(key) - k)[len(key) - k]
        if kth > 0:
            idx = idx[key >= kth * (1 - 1e-9)]
        else:
            idx = np.concatenate([idx[key > 0], idx[key == 0][:k]])
    items = [(int(numer[r]), int(denom[r]), int(r)) for r in idx]
    items.sort(key=functools.cmp_to_key(_cmp))
    return [it[2] for it in items[:k]]
