"""The definition of `mash cluster -R` / mg_cluster_tri_greedy_host in pure Python, for the tests.

An EDGE is a pair `mash triangle -E` prints under the same -d / -v (mg_compare_tri_results_host returns), as in
tests/cluster_model.py.  Walk the indices in order: i is a REPRESENTATIVE iff no representative j < i has an edge to i (the
lexicographically first maximal independent set of the graph); rep[i] is i for a representative and otherwise the smallest
representative j < i with an edge {i, j}.  `mash cluster -R` prints what `mash cluster` prints, cluster_model.cluster_stdout,
with rep in the labels' place: a representative precedes its members, clusters are numbered by ascending representative.

reps() is the sequential walk; reps_by_rounds() states the same a second way (brute force: repeated rounds to the first maximal
independent set, then the smallest adjacent representative); reps_fast() is the walk for millions of edges."""
from tests import cluster_model as cm


def _smaller_neighbours(n, rows, cols):
    nb = [[] for _ in range(n)]
    for r, c in zip(rows, cols):
        r, c = int(r), int(c)
        if r != c:
            nb[max(r, c)].append(min(r, c))
    return nb


def reps(n, rows, cols):
    """rep per index for the edges {rows[e], cols[e]}: the walk in index order"""
    nb = _smaller_neighbours(n, rows, cols)
    rep = list(range(n))
    for i in range(n):
        mine = [j for j in nb[i] if rep[j] == j]
        if mine:
            rep[i] = min(mine)
    return rep


def reps_by_rounds(n, rows, cols):
    """the same by brute force, nothing sequential in it: in every round an undecided index all of whose smaller neighbours are
    decided and none of them a representative becomes one, an undecided index beside a representative with a smaller index
    becomes a member; when nothing is undecided a member takes the smallest representative among ALL its neighbours that is
    smaller than itself"""
    edges = {(max(int(r), int(c)), min(int(r), int(c))) for r, c in zip(rows, cols) if int(r) != int(c)}
    state = [None] * n                                           # None: undecided, True: representative, False: member
    while any(s is None for s in state):
        before = list(state)
        for i in range(n):
            if before[i] is not None:
                continue
            lower = [lo for hi, lo in edges if hi == i]
            if any(before[lo] is True for lo in lower):
                state[i] = False
            elif all(before[lo] is False for lo in lower):
                state[i] = True
        assert state != before                                   # every round decides the smallest undecided index at least
    rep = []
    for i in range(n):
        if state[i]:
            rep.append(i)
        else:
            around = [lo for hi, lo in edges if hi == i] + [hi for hi, lo in edges if lo == i]
            rep.append(min(j for j in around if state[j] and j < i))
    return rep


def reps_fast(n, rows, cols):
    """reps() for millions of edges: numpy sorts the edges by larger end, the walk then runs over slices"""
    import numpy as np
    rows = np.asarray(rows, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    hi, lo = np.maximum(rows, cols), np.minimum(rows, cols)
    keep = hi != lo
    hi, lo = hi[keep], lo[keep]
    order = np.argsort(hi, kind="stable")
    hi, lo = hi[order], lo[order]
    start = np.searchsorted(hi, np.arange(n + 1))
    is_rep = np.zeros(n, dtype=bool)
    rep = np.arange(n, dtype=np.int64)
    for i in range(n):
        nb = lo[start[i]:start[i + 1]]
        if len(nb):
            r = nb[is_rep[nb]]
            if len(r):
                rep[i] = r.min()
                continue
        is_rep[i] = True
    return [int(x) for x in rep]


def greedy_stdout_of_triangle(stdout, names, shown=None):
    """what `mash cluster -R` prints where `mash triangle -E` (same options) printed the recorded text"""
    e = cm.edges_of_stdout(stdout, names)
    rep = reps(len(names), [x[0] for x in e], [x[1] for x in e])
    return cm.cluster_stdout(rep, names if shown is None else shown)


# ---- what a fixture must show to tell the greedy partition from everything near it

def members_beside_several_earlier_reps(rep, edges):
    """members with an edge to two or more representatives of smaller index: the 'first representative' rule decides"""
    n_before = {}
    for r, c in edges:
        hi, lo = max(r, c), min(r, c)
        if rep[hi] != hi and rep[lo] == lo:
            n_before[hi] = n_before.get(hi, 0) + 1
    return sorted(i for i, k in n_before.items() if k >= 2)


def members_beside_a_later_rep(rep, edges):
    """members with an edge to a representative of LARGER index: it must not take them"""
    return sorted({min(r, c) for r, c in edges if rep[min(r, c)] != min(r, c) and rep[max(r, c)] == max(r, c)})


def every_member_is_beside_its_rep(rep, edges):
    have = {(max(r, c), min(r, c)) for r, c in edges}
    return all(rep[i] == i or (rep[i] < i and (i, rep[i]) in have and rep[rep[i]] == rep[i]) for i in range(len(rep)))


def no_two_reps_share_an_edge(rep, edges):
    return not any(rep[r] == r and rep[c] == c for r, c in edges if r != c)
