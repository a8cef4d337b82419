"""tests/cluster_model.py (the definition of `mash cluster`) against a brute-force closure, on the recorded `mash triangle -E`
stdout of the REFERENCE CLI (tests/golden/cluster, made by tests/golden/make_cluster_golden.py) and on random graphs; and the
conditions the recording must meet, re-asserted on the recorded text alone."""
import json
import os
import random

from tests import cluster_model as cm

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cluster")


def fixture():
    cases = json.load(open(os.path.join(GOLD, "cases.json")))
    texts = {c["name"]: open(os.path.join(GOLD, c["name"] + ".out")).read() for c in cases["cases"]}
    return cases, texts


def test_model_against_brute_force_closure_on_the_fixture():
    cases, texts = fixture()
    names = cases["names"]
    for name, text in texts.items():
        e = cm.edges_of_stdout(text, names)
        assert all(r > c for r, c in e), name                      # lower triangle, as the reference prints it
        rows, cols = [x[0] for x in e], [x[1] for x in e]
        want = cm.labels_by_closure(len(names), rows, cols)
        assert cm.labels(len(names), rows, cols) == want, name
        assert cm.labels(len(names), rows[::-1], cols[::-1]) == want, name       # nothing depends on the order of the edges
        assert cm.labels_fast(len(names), rows, cols) == want, name


def test_model_against_brute_force_closure_on_random_graphs():
    rng = random.Random(20261017)
    for _ in range(60):
        n = rng.randint(1, 400)
        m = rng.choice([0, n // 3, n, 3 * n])
        fam = rng.randint(1, 12)
        e = []
        for _ in range(m):
            a, b = rng.randrange(n), rng.randrange(n)
            if a != b and a % fam == b % fam:
                e.append((max(a, b), min(a, b)))
        rows, cols = [x[0] for x in e], [x[1] for x in e]
        want = cm.labels_by_closure(n, rows, cols)
        assert cm.labels(n, rows, cols) == want
        assert cm.labels_fast(n, rows, cols) == want
    # a path listed in descending order, the longest chain there is
    n = 3000
    rows, cols = list(range(n - 1, 0, -1)), list(range(n - 2, -1, -1))
    assert cm.labels(n, rows, cols) == [0] * n and cm.labels_fast(n, rows, cols) == [0] * n


def test_printed_form():
    lab = [0, 1, 0, 3, 1, 0]
    assert cm.cluster_stdout(lab, list("abcdef")) == "1\t3\ta\n2\t2\tb\n1\t3\tc\n3\t1\td\n2\t2\te\n1\t3\tf\n"
    assert cm.cluster_stdout([], []) == ""


def test_recorded_fixture_meets_its_conditions():
    cases, texts = fixture()
    names = cases["names"]
    assert len(names) == 44 and len(set(names)) == 44 and len(set(cases["comments"])) == 44
    assert [c["options"] for c in cases["cases"]] == [["-d", "0.01"], ["-d", "0.02"], ["-d", "0.05"], ["-v", "1e-30"], ["-d", "0.11", "-v", "1e-37"]]
    edges = {k: cm.edges_of_stdout(t, names) for k, t in texts.items()}
    ok, why = cm.fixture_conditions(edges, len(names), "v")
    assert ok, why
    # (the filters nest: what -d 0.01 prints, -d 0.02 prints too; and the -v case prints fewer lines than there are pairs)
    assert set(edges["d1"]) < set(edges["d2"]) < set(edges["d3"])
    assert 0 < len(edges["v"]) < 44 * 43 // 2 and set(edges["dv"]) < set(edges["v"])
