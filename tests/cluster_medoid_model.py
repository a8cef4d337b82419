"""The definition of `mash cluster -M` / mg_cluster_tri_medoid_host in pure Python integers, for the tests.

An EDGE is a pair `mash triangle -E` prints under the same -d / -v, with the counts of its column 5, numer/denom.  The CLUSTERS
and their labels are those of `mash cluster` (tests/cluster_model.py: connected components, label = smallest row).
  weight(e) = floor(numer * 2^32 / max(denom, 1))    at most 2^32, because numer <= denom; 0/0 counts as 0/1
  score[i]  = the sum of weight(e) over all edges with an end at i; a pair of the cluster that is not an edge contributes 0
  medoid[i] = among the rows of i's cluster the one with the largest score; equal scores go to the smallest row; a row without
              an edge is its own medoid, with score 0.
No float appears here, and nothing depends on the order of the edges.

medoid() is the sequential statement; medoid_brute() states the same a second way (per cluster, a maximum over its members of a
freshly computed sum; it shares nothing with the first, not even the union-find); medoid_fast() is numpy, for millions of edges.
All three return (label, medoid, score).  `mash cluster -M` prints "<cluster number>\\t<cluster size>\\t<ID>\\t<medoid's ID>",
numbers and sizes as `mash cluster` without -M."""
from tests import cluster_model as cm
from tests import cluster_nearest_model as nm

ONE = 1 << 32


def weight(numer, denom):
    return int(numer) * ONE // max(int(denom), 1)


def medoid(n, rows, cols, numer, denom):
    """(label, medoid, score): scores by one pass over the edges, then per cluster the first row in index order that no later row beats"""
    lab = cm.labels(n, rows, cols)
    score = [0] * n
    for r, c, a, b in zip(rows, cols, numer, denom):
        w = weight(a, b)
        score[int(r)] += w
        score[int(c)] += w
    top = list(range(n))                                          # per label: the best row so far (the label itself at first: the smallest row)
    for i in range(n):
        if score[i] > score[top[lab[i]]]:
            top[lab[i]] = i
    return lab, [top[lab[i]] for i in range(n)], score


def medoid_brute(n, rows, cols, numer, denom):
    """the same by brute force: clusters by closure, then per cluster max over members of (sum over ALL edges that touch the member)"""
    edges = [(int(r), int(c), int(a), int(b)) for r, c, a, b in zip(rows, cols, numer, denom)]
    lab = cm.labels_by_closure(n, [e[0] for e in edges], [e[1] for e in edges])
    score, med = [], [None] * n
    for i in range(n):
        score.append(sum((a << 32) // (b if b else 1) for r, c, a, b in edges for end in (r, c) if end == i))
    for members in cm.clusters(lab).values():
        best = max(members, key=lambda i: (score[i], -i))
        for i in members:
            med[i] = best
    return lab, med, score


def medoid_fast(n, rows, cols, numer, denom):
    """medoid() for millions of edges (numpy, 64-bit integers: numer < 2^32, so numer << 32 fits a uint64)"""
    import numpy as np
    rows = np.asarray(rows, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    w = (np.asarray(numer, dtype=np.uint64) << np.uint64(32)) // np.maximum(np.asarray(denom, dtype=np.uint64), np.uint64(1))
    lab = np.asarray(cm.labels_fast(n, rows, cols), dtype=np.int64)
    score = np.zeros(n, dtype=np.uint64)
    np.add.at(score, rows, w)
    np.add.at(score, cols, w)
    order = np.lexsort((np.arange(n), np.iinfo(np.uint64).max - score, lab))      # by cluster, largest score first, then smaller row
    lead = np.ones(n, dtype=bool)
    lead[1:] = lab[order][1:] != lab[order][:-1]
    top = np.zeros(n, dtype=np.int64)
    top[lab[order][lead]] = order[lead]
    return [int(x) for x in lab], [int(x) for x in top[lab]], [int(x) for x in score]


def medoid_of_stdout(stdout, names):
    e = nm.counted_edges_of_stdout(stdout, names)
    return medoid(len(names), *[[x[k] for x in e] for k in range(4)])


def medoid_stdout(lab, med, shown):
    """what `mash cluster -M` prints; shown[i]: the name (or, with -C, the comment) of sketch i"""
    cl = cm.clusters(lab)
    number = {l: k + 1 for k, l in enumerate(sorted(cl))}
    return "".join(f"{number[lab[i]]}\t{len(cl[lab[i]])}\t{shown[i]}\t{shown[med[i]]}\n" for i in range(len(lab)))


def medoid_stdout_of_triangle(stdout, names, shown=None):
    """what `mash cluster -M` prints where `mash triangle -E` (same options) printed the recorded text"""
    lab, med, _ = medoid_of_stdout(stdout, names)
    return medoid_stdout(lab, med, names if shown is None else shown)


# ---- what a fixture must show to tell the medoid from the first member

def clusters_with_another_medoid(lab, med):
    """labels of the clusters whose medoid is not their first member"""
    return sorted({lab[i] for i in range(len(lab)) if med[i] != lab[i]})


def clusters_with_a_tie(lab, score):
    """labels of the clusters of two rows or more in which two or more rows share the top score: the smallest must win"""
    out = []
    for l, members in sorted(cm.clusters(lab).items()):
        top = max(score[i] for i in members)
        if len(members) >= 2 and sum(score[i] == top for i in members) >= 2:
            out.append(l)
    return out
