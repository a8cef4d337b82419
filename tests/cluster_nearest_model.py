"""The definition of `mash cluster -B` / mg_cluster_tri_nearest_host in pure Python, for the tests.

An EDGE is a pair `mash triangle -E` prints under the same -d / -v, with the counts of its column 5, numer/denom.  The
REPRESENTATIVES are those of `mash cluster -R` (tests/cluster_greedy_model.py: the walk in index order).  A member joins, among
ALL the representatives it has an edge to -- smaller or larger index --, the one whose edge has the larger fraction numer/denom;
fractions are compared by cross-multiplication in integers (denom == 0 counts as 0/1, as mash_amd/csrc/forest_key.h does), and
equal fractions, also under different denominators, go to the smaller representative.  No float appears here.

nearest() is the sequential statement on top of cluster_greedy_model.reps(); nearest_brute() states the same a second way
(per member, a maximum over all its edges by a comparator, nothing shared with the first); nearest_fast() is for millions of
edges.  `mash cluster -B` prints "<cluster number>\\t<cluster size>\\t<ID>\\t<representative's ID>", clusters numbered from 1 by
ascending representative."""
import functools

from tests import cluster_greedy_model as gm
from tests import cluster_model as cm


def better(numer_a, denom_a, rep_a, numer_b, denom_b, rep_b):
    """edge a (to representative rep_a) ranks strictly before edge b: forest_before with the representative as the tie-break"""
    l = int(numer_a) * (int(denom_b) or 1)
    r = int(numer_b) * (int(denom_a) or 1)
    return l > r or (l == r and rep_a < rep_b)


def nearest(n, rows, cols, numer, denom):
    """rep per index: the walk names the representatives, then every edge between a representative and a member offers"""
    first = gm.reps(n, rows, cols)
    is_rep = [first[i] == i for i in range(n)]
    rep = list(range(n))
    best = [None] * n                                            # per member (numer, denom) of the edge to rep[member]
    for r, c, a, b in zip(rows, cols, numer, denom):
        r, c = int(r), int(c)
        if r == c or is_rep[r] == is_rep[c]:
            continue
        member, centre = (c, r) if is_rep[r] else (r, c)
        if best[member] is None or better(a, b, centre, best[member][0], best[member][1], rep[member]):
            best[member] = (int(a), int(b))
            rep[member] = centre
    return rep


def nearest_brute(n, rows, cols, numer, denom):
    """the same by brute force: the representatives by rounds, then per member the maximum of a sort over all its neighbours"""
    first = gm.reps_by_rounds(n, rows, cols)
    reps = {i for i in range(n) if first[i] == i}
    rep = []
    for i in range(n):
        if i in reps:
            rep.append(i)
            continue
        offers = [(int(a), int(b), int(c) if int(r) == i else int(r)) for r, c, a, b in zip(rows, cols, numer, denom)
                  if int(r) != int(c) and i in (int(r), int(c))]
        offers = [o for o in offers if o[2] in reps]
        offers.sort(key=functools.cmp_to_key(lambda x, y: -1 if better(x[0], x[1], x[2], y[0], y[1], y[2]) else
                                             1 if better(y[0], y[1], y[2], x[0], x[1], x[2]) else 0))
        rep.append(offers[0][2])
    return rep


def nearest_fast(n, rows, cols, numer, denom):
    """nearest() for millions of edges whose denominators are below 2^21: numpy orders the edges by the 64-bit key of
    mash_amd/csrc/forest_key.h (numer << 42, integer-divided by denom: an exact order of the fractions there, no float)"""
    import numpy as np
    rows = np.asarray(rows, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    numer = np.asarray(numer, dtype=np.uint64)
    denom = np.asarray(denom, dtype=np.uint64)
    assert int(denom.max(initial=0)) < (1 << 21)
    first = np.asarray(gm.reps_fast(n, rows, cols), dtype=np.int64)
    is_rep = first == np.arange(n)
    keep = (rows != cols) & (is_rep[rows] != is_rep[cols])
    rows, cols, numer, denom = rows[keep], cols[keep], numer[keep], denom[keep]
    member = np.where(is_rep[rows], cols, rows)
    centre = np.where(is_rep[rows], rows, cols)
    key = (numer << np.uint64(42)) // np.maximum(denom, np.uint64(1))
    order = np.lexsort((centre, np.iinfo(np.uint64).max - key, member))       # by member, best key first, then smaller representative
    member, centre = member[order], centre[order]
    lead = np.ones(len(member), dtype=bool)
    lead[1:] = member[1:] != member[:-1]
    rep = np.arange(n, dtype=np.int64)
    rep[member[lead]] = centre[lead]
    return [int(x) for x in rep]


def counted_edges_of_stdout(stdout, names):
    """a recorded `mash triangle -E` stdout -> [(row, col, numer, denom)] in the order of its lines (column 5: numer/denom)"""
    at = {nm: i for i, nm in enumerate(names)}
    assert len(at) == len(names), "names must be distinct"
    out = []
    for ln in stdout.splitlines():
        f = ln.split("\t")
        a, b = f[4].split("/")
        out.append((at[f[0]], at[f[1]], int(a), int(b)))
    return out


def nearest_of_stdout(stdout, names):
    e = counted_edges_of_stdout(stdout, names)
    return nearest(len(names), *[[x[k] for x in e] for k in range(4)])


def nearest_stdout(rep, shown):
    """what `mash cluster -B` prints for these representatives; shown[i]: the name (or, with -C, the comment) of sketch i"""
    cl = cm.clusters(rep)
    number = {l: k + 1 for k, l in enumerate(sorted(cl))}
    return "".join(f"{number[rep[i]]}\t{len(cl[rep[i]])}\t{shown[i]}\t{shown[rep[i]]}\n" for i in range(len(rep)))


def nearest_stdout_of_triangle(stdout, names, shown=None):
    """what `mash cluster -B` prints where `mash triangle -E` (same options) printed the recorded text"""
    return nearest_stdout(nearest_of_stdout(stdout, names), names if shown is None else shown)


# ---- what a fixture must show to tell the nearest representative from the first one

def members_with_a_tie_for_best(rep, edges):
    """members whose best fraction is offered by two or more representatives: the smaller one must take them"""
    out = []
    for i in range(len(rep)):
        if rep[i] == i:
            continue
        offers = [(a, b) for r, c, a, b in edges if i in (r, c) and r != c and rep[c if r == i else r] == (c if r == i else r)]
        top = [o for o in offers if not any(better(p[0], p[1], 0, o[0], o[1], 0) for p in offers)]
        if len(top) >= 2:
            out.append(i)
    return out
