"""The definition of `mash cluster -D <m>` / mg_cluster_tri_density_host in pure Python, for the tests.

An EDGE is a pair `mash triangle -E` prints under the same -d / -v, with the counts of its column 5, numer/denom; deg(i) is the
number of edges with an end at i.  A CORE has deg(i) >= m.  The clusters of cores are the connected components of the cores under
the edges whose both ends are cores.  A BORDER is not a core and has an edge to a core; it joins the cluster of the core whose edge
has the larger fraction numer/denom -- compared by cross-multiplication in integers (denom == 0 counts as 0/1, as
mash_amd/csrc/forest_key.h does) --, equal fractions, also under different denominators, to the core of smaller row: via(i).
Edges between two rows that are not cores decide nothing.  Everything else is NOISE, a cluster of its own.  label[i] is the smallest
row of i's final cluster, borders included; via[i] is i for cores and noise.  No float appears here.

density() is the sequential statement; density_brute() states the same a second way (per row its neighbours by a scan, cores by
count, components by repeated relabelling, the border's choice by a sort under a comparator; nothing shared with the first);
density_fast() is for millions of edges.  All three return (label, via, degree).  `mash cluster -D` prints
"<cluster number>\\t<cluster size>\\t<ID>\\t<role>\\t<neighbours>", clusters numbered from 1 by first member."""
import functools


def better(numer_a, denom_a, core_a, numer_b, denom_b, core_b):
    """edge a (to core core_a) ranks strictly before edge b: forest_before with the core as the tie-break"""
    l = int(numer_a) * (int(denom_b) or 1)
    r = int(numer_b) * (int(denom_a) or 1)
    return l > r or (l == r and core_a < core_b)


def density(n, rows, cols, numer, denom, m):
    """(label, via, degree): degrees, a union-find over the core-core edges, every core-border edge offers, then the relabelling"""
    assert m >= 1
    edges = [(int(r), int(c), int(a), int(b)) for r, c, a, b in zip(rows, cols, numer, denom) if int(r) != int(c)]
    deg = [0] * n
    for r, c, _, _ in edges:
        deg[r] += 1
        deg[c] += 1
    core = [d >= m for d in deg]
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    via = list(range(n))
    best = [None] * n
    for r, c, a, b in edges:
        if core[r] and core[c]:
            x, y = find(r), find(c)
            if x != y:
                parent[max(x, y)] = min(x, y)
        elif core[r] != core[c]:
            member, centre = (c, r) if core[r] else (r, c)
            if best[member] is None or better(a, b, centre, best[member][0], best[member][1], via[member]):
                best[member] = (a, b)
                via[member] = centre
    root = [find(via[i]) for i in range(n)]
    first = {}
    for i in range(n):
        first.setdefault(root[i], i)
    return [first[root[i]] for i in range(n)], via, deg


def density_brute(n, rows, cols, numer, denom, m):
    """the same by brute force"""
    pairs = [(int(r), int(c), int(a), int(b)) for r, c, a, b in zip(rows, cols, numer, denom)]
    near = []
    for i in range(n):                                            # per row: (neighbour, numer, denom) by a scan
        near.append([(c if r == i else r, a, b) for r, c, a, b in pairs if r != c and i in (r, c)])
    deg = [len(x) for x in near]
    cores = {i for i in range(n) if deg[i] >= m}
    lab = list(range(n))                                          # the smallest core reachable over cores, by repeated relabelling
    changed = True
    while changed:
        changed = False
        for i in cores:
            for j, _, _ in near[i]:
                if j in cores and lab[j] < lab[i]:
                    lab[i] = lab[j]
                    changed = True
    via = list(range(n))
    for i in range(n):
        if i in cores:
            continue
        offers = [(a, b, j) for j, a, b in near[i] if j in cores]
        if offers:
            offers.sort(key=functools.cmp_to_key(lambda x, y: -1 if better(x[0], x[1], x[2], y[0], y[1], y[2]) else
                                                 1 if better(y[0], y[1], y[2], x[0], x[1], x[2]) else 0))
            via[i] = offers[0][2]
    group = [lab[via[i]] for i in range(n)]
    return [min(j for j in range(n) if group[j] == group[i]) for i in range(n)], via, deg


def density_fast(n, rows, cols, numer, denom, m):
    """density() for millions of edges whose denominators are below 2^21: numpy orders a border's edges by the 64-bit key of
    mash_amd/csrc/forest_key.h (numer << 42, integer-divided by denom: an exact order of the fractions there, no float)"""
    import numpy as np
    from tests import cluster_model as cm
    rows = np.asarray(rows, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    numer = np.asarray(numer, dtype=np.uint64)
    denom = np.asarray(denom, dtype=np.uint64)
    assert int(denom.max(initial=0)) < (1 << 21)
    keep = rows != cols
    rows, cols, numer, denom = rows[keep], cols[keep], numer[keep], denom[keep]
    deg = np.bincount(rows, minlength=n) + np.bincount(cols, minlength=n)
    core = deg >= m
    both = core[rows] & core[cols]
    lab = np.asarray(cm.labels_fast(n, rows[both], cols[both]), dtype=np.int64)
    one = core[rows] != core[cols]
    r1, c1 = rows[one], cols[one]
    member = np.where(core[r1], c1, r1)
    centre = np.where(core[r1], r1, c1)
    key = (numer[one] << np.uint64(42)) // np.maximum(denom[one], np.uint64(1))
    order = np.lexsort((centre, np.iinfo(np.uint64).max - key, member))       # by member, best key first, then smaller core
    member, centre = member[order], centre[order]
    lead = np.ones(len(member), dtype=bool)
    lead[1:] = member[1:] != member[:-1]
    via = np.arange(n, dtype=np.int64)
    via[member[lead]] = centre[lead]
    root = lab[via]
    first = np.full(n, n, dtype=np.int64)
    np.minimum.at(first, root, np.arange(n, dtype=np.int64))
    return [int(x) for x in first[root]], [int(x) for x in via], [int(x) for x in deg]


def roles(via, degree, m):
    """per row "core", "border" or "noise\""""
    return ["core" if degree[i] >= m else "border" if via[i] != i else "noise" for i in range(len(via))]


def figures(label, via, degree, m):
    """(clusters, cores, borders, noise)"""
    r = roles(via, degree, m)
    return sum(label[i] == i for i in range(len(label))), r.count("core"), r.count("border"), r.count("noise")


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


def density_of_stdout(stdout, names, m):
    e = counted_edges_of_stdout(stdout, names)
    return density(len(names), *[[x[k] for x in e] for k in range(4)], m)


def density_stdout(label, via, degree, m, shown):
    """what `mash cluster -D m` prints for these results; shown[i]: the name (or, with -C, the comment) of sketch i"""
    size = {}
    for l in label:
        size[l] = size.get(l, 0) + 1
    number = {l: k + 1 for k, l in enumerate(sorted(size))}
    r = roles(via, degree, m)
    return "".join(f"{number[label[i]]}\t{size[label[i]]}\t{shown[i]}\t{r[i]}\t{degree[i]}\n" for i in range(len(label)))


def density_stdout_of_triangle(stdout, names, m, shown=None):
    """what `mash cluster -D m` prints where `mash triangle -E` (same options) printed the recorded text"""
    return density_stdout(*density_of_stdout(stdout, names, m), m, names if shown is None else shown)


# ---- what a fixture must show to tell the rules apart

def borders_with_a_tie_for_best(via, degree, m, edges):
    """borders whose best fraction is offered by two or more cores: the smaller one must take them"""
    out = []
    for i in range(len(via)):
        if degree[i] >= m or via[i] == i:
            continue
        offers = [(a, b) for r, c, a, b in edges if r != c and i in (r, c) and degree[c if r == i else r] >= m]
        top = [o for o in offers if not any(better(p[0], p[1], 0, o[0], o[1], 0) for p in offers)]
        if len(top) >= 2:
            out.append(i)
    return out


def borders_first_in_their_cluster(label, via, degree, m):
    return [i for i in range(len(via)) if degree[i] < m and via[i] != i and label[i] == i]


def borders_under_a_later_core(via, degree, m):
    return [i for i in range(len(via)) if degree[i] < m and via[i] > i]


def borders_between_two_clusters(label, via, degree, m, edges):
    """borders with core neighbours in two or more clusters"""
    seen = {}
    for r, c, _, _ in edges:
        for i, j in ((r, c), (c, r)):
            if r != c and degree[i] < m and degree[j] >= m:
                seen.setdefault(i, set()).add(label[j])
    return [i for i, s in seen.items() if len(s) >= 2]
