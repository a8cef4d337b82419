"""The definition of `mash cluster` / mg_cluster_tri_host in pure Python, for the tests.

An EDGE is a pair `mash triangle -E` prints under the same -d / -v (mg_compare_tri_results_host returns); a CLUSTER is a
connected component of that graph (single linkage); label[i] is the smallest index in i's cluster.  `mash cluster` prints one
line per sketch in input order, "<cluster number>\\t<cluster size>\\t<name>", clusters numbered from 1 in order of their first
member, that is by ascending label.

labels() works on {row, col} arrays; edges_of_stdout() reads a recorded `mash triangle -E` stdout through its first two
columns and the names in input order (which must be distinct), so cluster_stdout_of_triangle() states what `mash cluster`
prints where `mash triangle -E` (same options) printed the recorded text."""


def labels(n, rows, cols):
    """label per index for the edges {rows[e], cols[e]}: a plain union-find that keeps the smaller root"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for r, c in zip(rows, cols):
        a, b = find(int(r)), find(int(c))
        if a != b:
            parent[max(a, b)] = min(a, b)
    return [find(i) for i in range(n)]


def labels_by_closure(n, rows, cols):
    """the same by brute force: label[i] = the smallest index reachable from i (repeated relaxation over the edges)"""
    lab = list(range(n))
    edges = [(int(r), int(c)) for r, c in zip(rows, cols)]
    changed = True
    while changed:
        changed = False
        for r, c in edges:
            m = min(lab[r], lab[c])
            if lab[r] != m or lab[c] != m:
                lab[r] = lab[c] = m
                changed = True
    return lab


def labels_fast(n, rows, cols):
    """labels() for millions of edges (numpy; the tests check it against labels()): every edge pulls both ends down to the smaller
    label of the two, labels then jump to their label's label, until nothing moves"""
    import numpy as np
    rows = np.asarray(rows, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    lab = np.arange(n, dtype=np.int64)
    while True:
        m = np.minimum(lab[rows], lab[cols])
        new = lab.copy()
        np.minimum.at(new, rows, m)
        np.minimum.at(new, cols, m)
        np.minimum.at(new, lab[rows], m)                          # (the ends' current labels follow too: whole groups move at once)
        np.minimum.at(new, lab[cols], m)
        while True:
            j = new[new]
            if np.array_equal(j, new):
                break
            new = j
        if np.array_equal(new, lab):
            return [int(x) for x in lab]
        lab = new


def edges_of_stdout(stdout, names):
    """a recorded `mash triangle -E` stdout -> [(row, col)] in the order of its lines"""
    at = {nm: i for i, nm in enumerate(names)}
    assert len(at) == len(names), "names must be distinct"
    out = []
    for ln in stdout.splitlines():
        f = ln.split("\t")
        out.append((at[f[0]], at[f[1]]))
    return out


def clusters(lab):
    """{label: [members ascending]}"""
    out = {}
    for i, l in enumerate(lab):
        out.setdefault(l, []).append(i)
    return out


def cluster_stdout(lab, shown):
    """what `mash cluster` prints for these labels; shown[i]: the name (or, with -C, the comment) of sketch i"""
    cl = clusters(lab)
    number = {l: k + 1 for k, l in enumerate(sorted(cl))}
    return "".join(f"{number[lab[i]]}\t{len(cl[lab[i]])}\t{shown[i]}\n" for i in range(len(lab)))


def cluster_stdout_of_triangle(stdout, names, shown=None):
    e = edges_of_stdout(stdout, names)
    lab = labels(len(names), [x[0] for x in e], [x[1] for x in e])
    return cluster_stdout(lab, names if shown is None else shown)


# ---- what the recorded fixture must show (tests/golden/make_cluster_golden.py asserts them, the test re-asserts them)

def non_clique_clusters(lab, edges):
    """labels of clusters in which some pair of members is not an edge: the chains that separate single linkage from the rest"""
    have = {(max(r, c), min(r, c)) for r, c in edges}
    return [l for l, m in clusters(lab).items() if any((b, a) not in have for i, a in enumerate(m) for b in m[i + 1:])]


def has_non_contiguous_cluster(lab):
    return any(m[-1] - m[0] + 1 != len(m) for m in clusters(lab).values())


def has_cluster_opened_away_from_its_smallest(lab, edges):
    """a cluster whose first edge, in the order given, joins two members neither of which is its smallest"""
    seen = set()
    for r, c in edges:
        if lab[r] not in seen:
            seen.add(lab[r])
            if lab[r] not in (r, c):
                return True
    return False


def fixture_conditions(case_edges, n, plain_v):
    """case_edges: {case name: [(row, col)]} with the three -d cases under "d1", "d2", "d3" and the -v case under `plain_v`.
    (met, why not)"""
    labs = {k: labels(n, [x[0] for x in e], [x[1] for x in e]) for k, e in case_edges.items()}
    if not any(non_clique_clusters(labs[k], case_edges[k]) for k in labs):
        return False, "(a) no cluster that is not a clique"
    def sizes(k):
        return sorted(len(m) for m in clusters(labs[k]).values())
    if not any(sizes(k).count(1) >= 2 and 2 in sizes(k) and sizes(k)[-1] >= 10 for k in labs):
        return False, "(b) no case with two singletons, a cluster of two and one of ten or more"
    if not any(has_non_contiguous_cluster(labs[k]) for k in labs):
        return False, "(c) every cluster is contiguous in input order"
    if not any(has_cluster_opened_away_from_its_smallest(labs[k], case_edges[k]) for k in labs):
        return False, "(c) every cluster's first edge touches its smallest member"
    if len({tuple(labs[k]) for k in ("d1", "d2", "d3")}) != 3:
        return False, "(d) the three -d cases do not give three partitions"
    if len(set(labs[plain_v])) in (1, n):
        return False, "(d) -v gives what no filter gives (one cluster), or no edge at all"
    return True, ""
