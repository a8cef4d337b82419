"""The definition of `mash cluster -L` / mg_cluster_tri_complete_host in pure Python, for the tests.

An EDGE is a pair `mash triangle -E` prints under the same -d / -v (mg_compare_tri_results_host returns): (row, col, numer, denom).
A cluster's ID is its smallest row; start from singletons.  Two clusters A, B are LINKED iff every pair {a in A, b in B} is an edge;
the link's WEIGHT is the worst of those edges, the smallest fraction numer/denom (0/0 counts as 0/1).  Links are ORDERED: larger
weight first, equal weights -- also under different denominators -- by ascending larger id, then ascending smaller id.  Repeat: merge
the first link, the new cluster keeps the smaller id; stop when no link is left.  label[i] = the id of i's final cluster.

walk() is that sentence, word for word, on Fractions: every step looks at every pair of clusters and at every pair of rows between
them.  rounds() is the second statement -- merge every MUTUAL link (the first link of both its clusters) at once, repeat -- and
returns how many rounds merged something.  walk_fast() keeps the links as a dict of adjacency under the integer key of
forest_model.key and a heap, for a few 10^5 edges.  complete_stdout_of_triangle() states what `mash cluster -L` prints where `mash
triangle -E` (same options) printed the recorded text."""
import heapq

from tests import cluster_model
from tests import forest_model

fraction = forest_model.fraction


def link_key(weight, a, b):
    """sorts links best first: weight a Fraction (or any number that orders as one), a and b the two cluster ids"""
    return (-weight, max(a, b), min(a, b))


def edge_weights(edges):
    """{(hi, lo): Fraction} of (row, col, numer, denom, ...) records"""
    out = {}
    for e in edges:
        out[(max(e[0], e[1]), min(e[0], e[1]))] = fraction(e[2], e[3])
    return out


def link_between(w, A, B):
    """the weight of the link between the member lists A and B, None if some pair between them is no edge"""
    worst = None
    for a in A:
        for b in B:
            x = w.get((max(a, b), min(a, b)))
            if x is None:
                return None
            if worst is None or x < worst:
                worst = x
    return worst


def walk(n, edges):
    """-> (label, merges): the sequential walk; merges = [(hi id, lo id)] in the order they were made"""
    w = edge_weights(edges)
    members = {i: [i] for i in range(n)}
    merges = []
    while True:
        best = None
        ids = sorted(members)
        for i, a in enumerate(ids):
            for b in ids[i + 1:]:
                x = link_between(w, members[a], members[b])
                if x is not None and (best is None or link_key(x, a, b) < best):
                    best = link_key(x, a, b)
        if best is None:
            break
        _, hi, lo = best
        members[lo] += members.pop(hi)
        merges.append((hi, lo))
    label = [0] * n
    for i, m in members.items():
        for x in m:
            label[x] = i
    return label, merges


def rounds(n, edges):
    """-> (label, merges as a set, rounds that merged something): every mutual link of a round is merged at once"""
    links = edge_weights(edges)                                    # between cluster ids from here on
    up = list(range(n))
    merges = set()
    count = 0
    while links:
        first = {}
        for (hi, lo), x in links.items():
            k = link_key(x, hi, lo)
            for end in (hi, lo):
                if end not in first or k < first[end]:
                    first[end] = k
        mate = {}
        for (hi, lo), x in links.items():
            k = link_key(x, hi, lo)
            if first[hi] == k and first[lo] == k:
                mate[hi], mate[lo] = lo, hi
                merges.add((hi, lo))
                up[hi] = lo
        assert mate, "the first link of all is mutual"
        count += 1
        nxt = {}
        for (hi, lo), x in links.items():
            if mate.get(hi, n) < hi or mate.get(lo, n) < lo:
                continue                                           # an absorbed end
            sides = [[end, mate[end]] if end in mate else [end] for end in (hi, lo)]
            parts = [links.get((max(a, b), min(a, b))) for a in sides[0] for b in sides[1]]
            if all(p is not None for p in parts):
                nxt[(hi, lo)] = min(parts)
        links = nxt

    def find(x):
        while up[x] != x:
            x = up[x]
        return x
    return [find(i) for i in range(n)], merges, count


def walk_fast(n, row, col, numer, denom):
    """walk() for a few 10^5 edges -> label: the links as adj[id] = {other id: key} under forest_model.key (exact below denominators
    of 2^21), the order as a heap of (-key, hi, lo) whose stale entries are dropped when they surface"""
    adj = [dict() for _ in range(n)]
    heap = []
    for r, c, a, b in zip(row, col, numer, denom):
        r, c, k = int(r), int(c), forest_model.key(int(a), int(b))
        assert int(b) < forest_model.DENOM_LIMIT
        adj[r][c] = adj[c][r] = k
        heap.append((-k, max(r, c), min(r, c)))
    heapq.heapify(heap)
    up = list(range(n))
    while heap:
        k, hi, lo = heapq.heappop(heap)
        if adj[hi].get(lo) != -k:
            continue                                               # (a link that died or whose weight dropped since)
        a, b = adj[lo], adj[hi]
        merged = {o: min(x, b[o]) for o, x in a.items() if o in b}
        for o in a:
            del adj[o][lo]
        for o in b:
            if o != lo:
                del adj[o][hi]
        for o, x in merged.items():
            adj[o][lo] = x
            heapq.heappush(heap, (-x, max(o, lo), min(o, lo)))
        adj[lo] = merged
        adj[hi] = {}
        up[hi] = lo
    for i in range(n):                                             # (links go from larger to smaller: one pass in index order)
        up[i] = up[up[i]]
    return up


def labels(n, edges):
    """walk_fast() over (row, col, numer, denom, ...) records"""
    return walk_fast(n, [e[0] for e in edges], [e[1] for e in edges], [e[2] for e in edges], [e[3] for e in edges])


def not_cliques(label, edges):
    """the ids of clusters in which some pair of members is no edge"""
    return cluster_model.non_clique_clusters(label, [(e[0], e[1]) for e in edges])


def linked_pairs(label, edges):
    """the pairs of final clusters that are still linked (every pair between them an edge): there must be none"""
    have = {(max(e[0], e[1]), min(e[0], e[1])) for e in edges}
    cl = cluster_model.clusters(label)
    touching = {(max(label[a], label[b]), min(label[a], label[b])) for a, b in have if label[a] != label[b]}
    return [(x, y) for x, y in sorted(touching) if all((max(a, b), min(a, b)) in have for a in cl[x] for b in cl[y])]


def complete_stdout_of_triangle(stdout, names, shown=None):
    """what `mash cluster -L` prints; shown: the comments where -C is given"""
    lab = labels(len(names), forest_model.lines_of_stdout(stdout, names))
    return cluster_model.cluster_stdout(lab, names if shown is None else shown)
