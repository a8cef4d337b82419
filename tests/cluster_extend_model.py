"""The definitions of `mash cluster -A` / mg_cluster_extend_host / mg_cluster_extend_greedy_host in pure Python, for the tests.

ref has n rows with an earlier result, qry m rows; `cat` is ref's rows followed by qry's, new row q has index n + q.  A NEW EDGE
is an edge of cat's thresholded triangle (tests/cluster_model.py) that touches a new row, given here in cat's index space.

extend_labels(): ref_label[i] <= i and ref_label[ref_label[i]] == ref_label[i]; the result is the connected components of the
graph {i ~ ref_label[i]} + new edges over all n + m rows, each labelled by its smallest row.
extend_reps(): ref_rep in the same form, or None (every row of ref is a representative); the old rows stay what they are and the
walk in index order goes on over the new rows: a new row is a representative iff no representative with a smaller index has a
new edge to it, else it joins the smallest such.  The result holds the new rows only, values in cat's index space.

new_edges() picks the edges that touch a row >= n; check_seed() states the two conditions; earlier_of_stdout() reads an earlier
`mash cluster` stdout the way the command does."""


def check_seed(seed):
    """the first row that breaks one of the two conditions, or None"""
    for i, s in enumerate(seed):
        if s > i or seed[s] != s:
            return i
    return None


def new_edges(edges, n):
    return [(r, c) for r, c in edges if max(r, c) >= n]


def extend_labels(n, m, ref_label, edges):
    """label per row of cat; every edge must touch a new row"""
    assert len(ref_label) == n and check_seed(ref_label) is None
    parent = list(range(n + m))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    def unite(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)

    for i, l in enumerate(ref_label):
        unite(i, int(l))
    for r, c in edges:
        assert max(r, c) >= n
        unite(int(r), int(c))
    return [find(i) for i in range(n + m)]


def extend_reps(n, m, ref_rep, edges):
    """rep of the m new rows, in cat's index space"""
    if ref_rep is not None:
        assert len(ref_rep) == n and check_seed(ref_rep) is None
    is_rep = [ref_rep is None or int(ref_rep[i]) == i for i in range(n)] + [False] * m
    nb = [[] for _ in range(m)]
    for r, c in edges:
        r, c = int(r), int(c)
        assert max(r, c) >= n
        if r != c:
            nb[max(r, c) - n].append(min(r, c))
    rep = []
    for q in range(m):
        mine = [j for j in nb[q] if is_rep[j]]
        rep.append(min(mine) if mine else n + q)
        is_rep[n + q] = not mine
    return rep


def earlier_of_stdout(text):
    """an earlier `mash cluster` stdout -> (label per line = the first line that carries its number, ID per line)"""
    first, label, ids = {}, [], []
    for ln in text.splitlines():
        number, _, shown = ln.split("\t", 2)
        assert number.isdigit() and int(number) > 0
        label.append(first.setdefault(int(number), len(label)))
        ids.append(shown)
    return label, ids
