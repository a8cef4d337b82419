"""tests/cluster_density_model.py (the definition of `mash cluster -D`): the sequential statement against the brute-force one and the
numpy one on random graphs with counts, the properties the definition promises, -D 1 against single linkage, and the figures of
the recorded `mash triangle -E` stdout of the REFERENCE CLI (tests/golden/cluster), asserted on the recorded text alone."""
import inspect
import io
import json
import os
import random
import tokenize

import pytest

from tests import cluster_density_model as dm
from tests import cluster_model as cm

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cluster")

# (case, m) -> (clusters, cores, borders, noise); whether the partition is single linkage's
PINS = {("d1", 3): (34, 8, 4, 32), ("d2", 3): (18, 25, 5, 14), ("d2", 6): (23, 11, 13, 20), ("d3", 10): (25, 6, 14, 24),
        ("v", 38): (5, 19, 21, 4), ("dv", 35): (5, 19, 21, 4)}
SAME_PARTITION = {("v", 38), ("dv", 35)}


def fixture():
    cases = json.load(open(os.path.join(GOLD, "cases.json")))
    texts = {c["name"]: open(os.path.join(GOLD, c["name"] + ".out")).read() for c in cases["cases"]}
    return cases, texts


def columns(e):
    return [[x[k] for x in e] for k in range(4)]


def random_graph(rng):
    n = rng.randint(1, 90)
    fam = rng.randint(1, 4)
    seen, e = set(), []
    for _ in range(rng.choice([0, n // 3, n, 3 * n, 8 * n])):
        a, b = rng.randrange(n), rng.randrange(n)
        if a != b and (a % fam == b % fam or rng.randrange(6) == 0) and (max(a, b), min(a, b)) not in seen:      # a few bridges between families
            seen.add((max(a, b), min(a, b)))
            d = rng.choice([0, 32, 64, 64, 64])                                   # quarters of 64 and 32, and 0/0: ties across denominators
            e.append((a, b, rng.randint(0, 4) * (d // 4), d))
    return n, e


def test_three_statements_agree_on_random_graphs_and_keep_their_promises():
    rng = random.Random(20261021)
    ties = between = 0
    for _ in range(120):
        n, e = random_graph(rng)
        deg_max = max([0] + dm.density(n, *columns(e), 1)[2])
        cores_before = None
        for m in sorted({1, 2, 3, max(1, deg_max // 2), max(1, deg_max), deg_max + 1}):
            want = dm.density_brute(n, *columns(e), m)
            assert dm.density(n, *columns(e), m) == want
            assert dm.density_fast(n, *columns(e), m) == want
            rev = [(c, r, a, b) for r, c, a, b in reversed(e)]                    # neither the order nor the orientation of the edges matters
            assert dm.density(n, *columns(rev), m) == want
            label, via, deg = want
            cores = {i for i in range(n) if deg[i] >= m}
            assert cores_before is None or cores <= cores_before                 # cores at a larger m are a subset
            cores_before = cores
            have = {(max(r, c), min(r, c)) for r, c, _, _ in e}
            for i in range(n):
                assert label[label[i]] == label[i] <= i
                if via[i] != i:                                                  # a border: an edge to via, and via is a core
                    assert i not in cores and via[i] in cores and (max(i, via[i]), min(i, via[i])) in have and label[i] == label[via[i]]
            for r, c, _, _ in e:                                                 # no edge joins cores of two clusters
                assert not (r in cores and c in cores) or label[r] == label[c]
            if m == 1:
                assert label == cm.labels(n, [x[0] for x in e], [x[1] for x in e]) and via == list(range(n))
            if m == deg_max + 1:
                assert label == list(range(n)) == via
            ties += bool(dm.borders_with_a_tie_for_best(via, deg, m, e))
            between += bool(dm.borders_between_two_clusters(label, via, deg, m, e))
    assert ties >= 20 and between >= 20                                          # the graphs do tell the rules apart


def test_shapes_with_a_known_answer():
    # two triangles 0-1-2 and 4-5-6 and a bridge row 3 with one edge to each, nearer the later one
    tri = [(1, 0, 60, 64), (2, 0, 60, 64), (2, 1, 60, 64), (5, 4, 60, 64), (6, 4, 60, 64), (6, 5, 60, 64)]
    later = tri + [(3, 2, 30, 64), (4, 3, 31, 64)]
    # (row 3 has two edges: at m = 2 it is a core and chains the two; at m = 3 only rows 2 and 4 are cores, everything else a border)
    assert dm.density(7, *columns(later), 2) == ([0] * 7, list(range(7)), [2, 2, 3, 2, 3, 2, 2])
    assert dm.density(7, *columns(later), 3)[:2] == ([0, 0, 0, 3, 3, 3, 3], [2, 2, 2, 4, 4, 4, 4])
    far = [(i, j, 60, 64) for i in range(4) for j in range(i)] + [(i, j, 60, 64) for i in range(5, 9) for j in range(5, i)]
    for e, v in (([(4, 3, 30, 64), (5, 4, 31, 64)], 5), ([(4, 3, 31, 64), (5, 4, 30, 64)], 3), ([(4, 3, 32, 64), (5, 4, 16, 32)], 3),
                 ([(4, 3, 16, 32), (5, 4, 32, 64)], 3), ([(4, 3, 0, 64), (5, 4, 0, 0)], 3), ([(4, 3, 0, 0), (5, 4, 0, 64)], 3)):
        label, via, deg = dm.density(9, *columns(far + e), 3)
        assert via == [0, 1, 2, 3, v, 5, 6, 7, 8] and deg[4] == 2
        assert label == ([0] * 5 + [5] * 4 if v == 3 else [0] * 4 + [4] * 5)     # under the later core the border names the cluster
        assert dm.density_brute(9, *columns(far + e), 3) == (label, via, deg) == dm.density_fast(9, *columns(far + e), 3)
    # two rows that are not cores, joined to each other and to cores of different clusters: the clusters stay apart
    e = far + [(4, 3, 10, 64), (9, 5, 10, 64), (9, 4, 64, 64)]
    label, via, deg = dm.density(10, *columns(e), 3)
    assert (via[4], via[9], label[4], label[9]) == (3, 5, 0, 5) and label[0] != label[5]
    # a row whose only edges go to rows that are not cores is noise
    label, via, deg = dm.density(12, *columns(e + [(11, 10, 64, 64)]), 3)
    assert (via[10], via[11], label[10], label[11], deg[10], deg[11]) == (10, 11, 10, 11, 1, 1)
    assert dm.roles(via, deg, 3) == ["core"] * 4 + ["border"] + ["core"] * 4 + ["border", "noise", "noise"]
    assert dm.density(0, [], [], [], [], 1) == ([], [], []) == dm.density_fast(0, [], [], [], [], 1)
    assert dm.density(1, [], [], [], [], 1) == ([0], [0], [0]) == dm.density_brute(1, [], [], [], [], 1)


def test_printed_form():
    names = ["a", "b", "c", "d", "e"]
    text = "b\ta\t0\t0\t5/9\nc\tb\t0\t0\t6/9\nd\tc\t0\t0\t1/1\nd\tb\t0\t0\t1/2\n"     # degrees a 1, b 3, c 2, d 2, e 0
    assert dm.density_stdout_of_triangle(text, names, 2) == "1\t4\ta\tborder\t1\n1\t4\tb\tcore\t3\n1\t4\tc\tcore\t2\n1\t4\td\tcore\t2\n2\t1\te\tnoise\t0\n"
    assert dm.density_stdout_of_triangle(text, names, 3, ["A", "B", "C", "D", "E"]) == \
        "1\t4\tA\tborder\t1\n1\t4\tB\tcore\t3\n1\t4\tC\tborder\t2\n1\t4\tD\tborder\t2\n2\t1\tE\tnoise\t0\n"
    one = dm.density_stdout_of_triangle(text, names, 1)
    assert ["\t".join(ln.split("\t")[:3]) + "\n" for ln in one.splitlines()] == cm.cluster_stdout_of_triangle(text, names).splitlines(True)
    assert dm.density_stdout_of_triangle(text, names, 4) == "".join(f"{i + 1}\t1\t{nm}\tnoise\t{d}\n" for i, (nm, d) in enumerate(zip(names, (1, 3, 2, 2, 0))))


def test_no_float_in_the_model():
    """the code of the model (comments and strings apart) has no true division, no float literal and no name with `float` in it"""
    toks = list(tokenize.generate_tokens(io.StringIO(inspect.getsource(dm)).readline))
    assert len(toks) > 500
    for t in toks:
        assert not (t.type == tokenize.OP and t.string in ("/", "/=")), t
        assert not (t.type == tokenize.NAME and "float" in t.string), t
        assert not (t.type == tokenize.NUMBER and not t.string.isdigit()), t


@pytest.mark.parametrize("name,m", sorted(PINS))
def test_figures_of_the_recorded_family(name, m):
    cases, texts = fixture()
    names = cases["names"]
    n = len(names)
    assert n == 44
    e = dm.counted_edges_of_stdout(texts[name], names)
    got = dm.density(n, *columns(e), m)
    assert dm.density_brute(n, *columns(e), m) == got == dm.density_fast(n, *columns(e), m)
    assert dm.figures(*got, m) == PINS[(name, m)]
    single = cm.labels(n, [x[0] for x in e], [x[1] for x in e])
    assert (got[0] == single) == ((name, m) in SAME_PARTITION)
    assert got[1] != list(range(n))                                              # roles and via differ from the plain run's in every case


def test_recorded_family_at_one_neighbour_is_plain_cluster():
    cases, texts = fixture()
    names = cases["names"]
    for name, text in texts.items():
        e = dm.counted_edges_of_stdout(text, names)
        label, via, deg = dm.density(len(names), *columns(e), 1)
        assert label == cm.labels(len(names), [x[0] for x in e], [x[1] for x in e]) and via == list(range(len(names))), name
        want = cm.cluster_stdout_of_triangle(text, names)
        got = dm.density_stdout_of_triangle(text, names, 1)
        assert "".join("\t".join(ln.split("\t")[:3]) + "\n" for ln in got.splitlines()) == want, name
        assert "border" not in got


def test_recorded_family_tells_the_relabelling_and_the_later_core_apart():
    cases, texts = fixture()
    names = cases["names"]
    e = dm.counted_edges_of_stdout(texts["d2"], names)
    label, via, deg = dm.density(len(names), *columns(e), 6)
    assert len(dm.borders_first_in_their_cluster(label, via, deg, 6)) > 0
    assert len(dm.borders_under_a_later_core(via, deg, 6)) > 0
