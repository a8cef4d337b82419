"""The definition of `mash cluster -T` / mg_cluster_tri_forest_host in pure Python, for the tests.

An EDGE is a pair `mash triangle -E` prints under the same -d / -v (mg_compare_tri_results_host returns): (row, col, numer, denom),
col < row.  ORDER: edge a before edge b iff numer_a * denom_b > numer_b * denom_a (0/0, two empty sketches, counts as 0/1); equal
fractions, also under different denominators, by ascending row, then ascending col -- a stable sort of the reference's stdout by
column 5 as a fraction, descending.  FOREST: walk the edges in that order, keep an edge iff its ends are not yet connected by kept
edges (Kruskal); the order is strict, so it is the one minimum spanning forest.  `mash cluster -T` prints the kept lines in that
order.

forest() is Kruskal on (row, col, numer, denom) tuples; forest_brute() the second statement of the same thing -- an edge is in the
forest iff its ends are NOT connected by the edges strictly before it; forest_fast() the numpy form for millions of records;
forest_stdout_of_triangle() states what `mash cluster -T` prints where `mash triangle -E` (same options) printed the recorded text;
key() is the 64-bit weight key of mash_amd/csrc/forest_key.h."""
from fractions import Fraction

DENOM_LIMIT = 1 << 21


def fraction(numer, denom):
    return Fraction(int(numer), int(denom) if denom else 1)


def order_key(e):
    """sorts (row, col, numer, denom) best first"""
    return (-fraction(e[2], e[3]), e[0], e[1])


def before(a, b):
    """the comparison as the code makes it: cross-multiplication in integers"""
    l, r = a[2] * (b[3] or 1), b[2] * (a[3] or 1)
    return l > r or (l == r and (a[0], a[1]) < (b[0], b[1]))


def key(numer, denom):
    """floor(numer * 2^42 / denom): orders as the fraction does for denominators below 2^21"""
    return (int(numer) << 42) // (int(denom) if denom else 1)


def kruskal(n, edges_in_order):
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    kept = []
    for e in edges_in_order:
        a, b = find(e[0]), find(e[1])
        if a != b:
            parent[max(a, b)] = min(a, b)
            kept.append(e)
    return kept


def forest(n, edges):
    """the forest's edges, best first"""
    return kruskal(n, sorted(edges, key=order_key))


def forest_brute(n, edges):
    """the same without a union-find and without a sort: an edge belongs to the forest iff its ends are not connected by the edges
    that rank strictly before it (a search over those edges, per edge)"""
    kept = []
    for e in edges:
        adj = {}
        for f in edges:
            if before(f, e):
                adj.setdefault(f[0], []).append(f[1])
                adj.setdefault(f[1], []).append(f[0])
        seen, todo = {e[0]}, [e[0]]
        while todo:
            for y in adj.get(todo.pop(), ()):
                if y not in seen:
                    seen.add(y)
                    todo.append(y)
        if e[1] not in seen:
            kept.append(e)
    out = []
    for e in kept:                                                 # best first, by insertion under before()
        at = 0
        while at < len(out) and before(out[at], e):
            at += 1
        out.insert(at, e)
    return out


def forest_fast(n, row, col, numer, denom):
    """forest() over numpy arrays of millions of records: -> indices into the records, best first.  The order is exact: the distinct
    {numer, denom} pairs (there are few) are ranked as Fractions, the records by (that rank, row, col).  Kruskal then runs over the
    sorted records in chunks: a chunk's edges whose ends already share a label are dropped at once, only the others are walked."""
    import numpy as np
    row = np.asarray(row, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    numer = np.asarray(numer, dtype=np.int64)
    denom = np.asarray(denom, dtype=np.int64)
    if len(row) == 0:
        return np.zeros(0, dtype=np.int64)
    pair = numer << 32 | denom
    uniq, inv = np.unique(pair, return_inverse=True)
    by_frac = sorted(range(len(uniq)), key=lambda u: -fraction(int(uniq[u]) >> 32, int(uniq[u]) & 0xFFFFFFFF))
    rank_of = np.zeros(len(uniq), dtype=np.int64)
    r = -1
    last = None
    for u in by_frac:                                              # equal fractions under different denominators share a rank
        f = fraction(int(uniq[u]) >> 32, int(uniq[u]) & 0xFFFFFFFF)
        if f != last:
            r += 1
            last = f
        rank_of[u] = r
    order = np.lexsort((col, row, rank_of[inv]))
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    kept = []
    chunk = max(4 * n, 1024)
    for lo in range(0, len(order), chunk):
        idx = order[lo:lo + chunk]
        lab = np.array(parent, dtype=np.int64)
        while True:
            nxt = lab[lab]
            if np.array_equal(nxt, lab):
                break
            lab = nxt
        idx = idx[lab[row[idx]] != lab[col[idx]]]
        for i in idx.tolist():
            a, b = find(int(row[i])), find(int(col[i]))
            if a != b:
                parent[max(a, b)] = min(a, b)
                kept.append(i)
    return np.array(kept, dtype=np.int64)


def lines_of_stdout(stdout, names):
    """a recorded `mash triangle -E` stdout -> [(row, col, numer, denom, line)] in the order of its lines"""
    at = {nm: i for i, nm in enumerate(names)}
    assert len(at) == len(names), "names must be distinct"
    out = []
    for ln in stdout.splitlines():
        f = ln.split("\t")
        numer, denom = f[4].split("/")
        out.append((at[f[0]], at[f[1]], int(numer), int(denom), ln))
    return out


def forest_lines(stdout, names):
    """the forest's records of a recorded stdout, best first: a STABLE sort of the lines by column 5, then Kruskal"""
    lines = lines_of_stdout(stdout, names)
    return kruskal(len(names), sorted(lines, key=lambda e: -fraction(e[2], e[3])))


def forest_stdout_of_triangle(stdout, names, shown=None):
    """what `mash cluster -T` prints; shown: the comments where -C is given (the recorded text carries the names)"""
    out = []
    for row, col, _, _, ln in forest_lines(stdout, names):
        f = ln.split("\t")
        if shown is not None:
            f[0], f[1] = shown[row], shown[col]
        out.append("\t".join(f) + "\n")
    return "".join(out)


def cut(forest_edges, numer, denom):
    """the forest's edges whose fraction is at least numer/denom: the forest of that stricter threshold"""
    return [e for e in forest_edges if fraction(e[2], e[3]) >= fraction(numer, denom)]
