"""tests/cluster_greedy_model.py (the definition of `mash cluster -R`): the sequential walk against a brute-force statement of
the same (rounds to the first maximal independent set, then the smallest adjacent representative), on the recorded `mash
triangle -E` stdout of the REFERENCE CLI (tests/golden/cluster) and on random graphs; and the conditions that make the
recording decisive for the greedy partition, asserted on the recorded text alone."""
import json
import os
import random

from tests import cluster_greedy_model as gm
from tests import cluster_model as cm

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cluster")


def fixture():
    cases = json.load(open(os.path.join(GOLD, "cases.json")))
    texts = {c["name"]: open(os.path.join(GOLD, c["name"] + ".out")).read() for c in cases["cases"]}
    return cases, texts


def test_walk_against_brute_force_rounds_on_the_fixture():
    cases, texts = fixture()
    names = cases["names"]
    for name, text in texts.items():
        e = cm.edges_of_stdout(text, names)
        rows, cols = [x[0] for x in e], [x[1] for x in e]
        want = gm.reps_by_rounds(len(names), rows, cols)
        assert gm.reps(len(names), rows, cols) == want, name
        assert gm.reps(len(names), cols[::-1], rows[::-1]) == want, name         # neither the order nor the orientation of the edges matters
        assert gm.reps_fast(len(names), rows, cols) == want, name


def test_walk_against_brute_force_rounds_on_random_graphs():
    rng = random.Random(20261017)
    for _ in range(60):
        n = rng.randint(1, 250)
        m = rng.choice([0, n // 3, n, 3 * n, 8 * n])
        fam = rng.randint(1, 12)
        e = []
        for _ in range(m):
            a, b = rng.randrange(n), rng.randrange(n)
            if a != b and a % fam == b % fam:
                e.append((a, b) if rng.random() < 0.5 else (b, a))
        rows, cols = [x[0] for x in e], [x[1] for x in e]
        want = gm.reps_by_rounds(n, rows, cols)
        assert gm.reps(n, rows, cols) == want
        assert gm.reps_fast(n, rows, cols) == want
        assert gm.every_member_is_beside_its_rep(want, e) and gm.no_two_reps_share_an_edge(want, e)


def test_shapes_with_a_known_answer():
    n = 2001
    path = [(i, i - 1) for i in range(1, n)]
    rows, cols = [x[0] for x in path], [x[1] for x in path]
    want = [i if i % 2 == 0 else i - 1 for i in range(n)]                        # every other row of a path in index order
    assert gm.reps(n, rows, cols) == want and gm.reps_fast(n, rows, cols) == want
    star = [(max(i, 7), min(i, 7)) for i in range(20) if i != 7]                 # a star around row 7 of 20
    rows, cols = [x[0] for x in star], [x[1] for x in star]
    # rows 0 .. 6 are representatives, 7 joins the first of them, rows 8 .. 19 have lost their centre: it collects nobody
    assert gm.reps(20, rows, cols) == [0, 1, 2, 3, 4, 5, 6, 0] + list(range(8, 20)) == gm.reps_by_rounds(20, rows, cols)
    band = [(i, i - k) for i in range(60) for k in (1, 2, 3) if i - k >= 0]
    rows, cols = [x[0] for x in band], [x[1] for x in band]
    assert gm.reps(60, rows, cols) == [i - i % 4 for i in range(60)]
    assert gm.reps(0, [], []) == [] and gm.reps(1, [], []) == [0] and gm.reps_fast(0, [], []) == []


def test_printed_form():
    names = ["a", "b", "c", "d"]
    text = "b\ta\t0\t0\t1/1\nc\tb\t0\t0\t1/1\nd\tc\t0\t0\t1/1\n"                  # the path a - b - c - d
    assert gm.greedy_stdout_of_triangle(text, names) == "1\t2\ta\n1\t2\tb\n2\t2\tc\n2\t2\td\n"
    assert cm.cluster_stdout_of_triangle(text, names) == "1\t4\ta\n1\t4\tb\n1\t4\tc\n1\t4\td\n"
    assert gm.greedy_stdout_of_triangle(text, names, ["A", "B", "C", "D"]) == "1\t2\tA\n1\t2\tB\n2\t2\tC\n2\t2\tD\n"


def test_recorded_fixture_is_decisive_for_the_greedy_partition():
    """on every recorded case the greedy partition is not the single-linkage one; members within the threshold of several
    earlier representatives (the first one takes them) and of a later one (it does not) both occur"""
    cases, texts = fixture()
    names = cases["names"]
    n = len(names)
    n_clusters, several, later = {}, {}, {}
    for name, text in texts.items():
        e = cm.edges_of_stdout(text, names)
        rows, cols = [x[0] for x in e], [x[1] for x in e]
        rep = gm.reps(n, rows, cols)
        single = cm.labels(n, rows, cols)
        assert rep != single, name
        n_clusters[name] = (len(set(rep)), len(set(single)))
        assert gm.every_member_is_beside_its_rep(rep, e), name
        assert gm.no_two_reps_share_an_edge(rep, e), name
        assert all(single[i] == single[rep[i]] for i in range(n)), name          # the greedy partition refines the single-linkage one
        several[name] = len(gm.members_beside_several_earlier_reps(rep, e))
        later[name] = len(gm.members_beside_a_later_rep(rep, e))
    assert n_clusters == {"d1": (31, 29), "d2": (22, 16), "d3": (8, 7), "v": (6, 5), "dv": (8, 5)}
    assert several == {"d1": 1, "d2": 12, "d3": 0, "v": 32, "dv": 26} and later == {"d1": 2, "d2": 0, "d3": 0, "v": 0, "dv": 9}
    assert any(several.values()) and any(later.values())
