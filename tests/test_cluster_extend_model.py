"""tests/cluster_extend_model.py (the definitions behind `mash cluster -A`) against the whole-table models
(tests/cluster_model.py, tests/cluster_greedy_model.py) on the recorded `mash triangle -E` stdout of the REFERENCE CLI
(tests/golden/cluster): for every recorded case and every split L in {0, 1, 17, 43, 44}, extending the model's partition of
the first L sketches by the recorded edges that touch a later one gives what the whole-table model gives on all recorded
edges; the same in three steps (10 -> 30 -> 44), with only the representatives kept as the earlier rows, and through the
text `mash cluster` prints (which is what -A reads back)."""
import json
import os
import random

from tests import cluster_extend_model as em
from tests import cluster_greedy_model as gm
from tests import cluster_model as cm

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cluster")
SPLITS = (0, 1, 17, 43, 44)


def fixture():
    cases = json.load(open(os.path.join(GOLD, "cases.json")))
    names = cases["names"]
    return names, {c["name"]: cm.edges_of_stdout(open(os.path.join(GOLD, c["name"] + ".out")).read(), names) for c in cases["cases"]}


def whole(n, edges, greedy):
    e = [(r, c) for r, c in edges if max(r, c) < n]
    return (gm.reps if greedy else cm.labels)(n, [x[0] for x in e], [x[1] for x in e])


def test_every_recorded_case_at_every_split():
    names, cases = fixture()
    n = len(names)
    assert n == 44 and len(cases) == 5
    for name, edges in cases.items():
        want_lab, want_rep = whole(n, edges, False), whole(n, edges, True)
        for L in SPLITS:
            new = em.new_edges(edges, L)
            assert len(new) + len([e for e in edges if max(e) < L]) == len(edges)
            assert em.extend_labels(L, n - L, whole(L, edges, False), new) == want_lab, (name, L)
            assert em.extend_labels(L, n - L, whole(L, edges, False), new[::-1]) == want_lab, (name, L)      # no order matters
            old_rep = whole(L, edges, True)
            assert old_rep == want_rep[:L], (name, L)                # the old rows never change
            assert em.extend_reps(L, n - L, old_rep, new) == want_rep[L:], (name, L)
            assert em.extend_reps(L, n - L, old_rep, new[::-1]) == want_rep[L:], (name, L)


def test_three_steps_give_the_one_shot_result():
    names, cases = fixture()
    n = len(names)
    for name, edges in cases.items():
        lab, rep = whole(10, edges, False), whole(10, edges, True)
        for a, b in ((10, 30), (30, 44)):
            step = [e for e in em.new_edges(edges, a) if max(e) < b]
            lab = em.extend_labels(a, b - a, lab, step)
            rep = rep + em.extend_reps(a, b - a, rep, step)
        assert lab == whole(n, edges, False) and rep == whole(n, edges, True), name


def test_representatives_alone_are_enough():
    """edges from a new row to an old member decide nothing: ref reduced to its representatives, ref_rep None, indices mapped back"""
    names, cases = fixture()
    n = len(names)
    for name, edges in cases.items():
        want = whole(n, edges, True)
        for L in SPLITS:
            old = whole(L, edges, True)
            keep = [i for i in range(L) if old[i] == i]
            at = {i: k for k, i in enumerate(keep)}
            at.update({i: len(keep) + (i - L) for i in range(L, n)})
            back = keep + list(range(L, n))
            small = [(at[r], at[c]) for r, c in em.new_edges(edges, L) if r in at and c in at]
            got = em.extend_reps(len(keep), n - L, None, small)
            assert [back[x] for x in got] == want[L:], (name, L)


def test_through_the_text_the_command_prints():
    names, cases = fixture()
    n = len(names)
    for name, edges in cases.items():
        for greedy in (False, True):
            for L in SPLITS:
                old = whole(L, edges, greedy)
                label, ids = em.earlier_of_stdout(cm.cluster_stdout(old, names[:L]))
                assert label == old and ids == names[:L], (name, greedy, L)      # the label is the first line with the number


def test_seed_conditions_and_random_graphs():
    assert em.check_seed([0, 0, 2, 2]) is None and em.check_seed([]) is None
    assert em.check_seed([0, 2, 2]) == 1                               # larger than its row
    assert em.check_seed([0, 0, 1]) == 2                               # not the first row of its cluster
    rng = random.Random(20261020)
    for _ in range(60):
        n = rng.randint(0, 200)
        m = rng.randint(0, 200)
        fam = rng.randint(1, 9)
        edges = []
        for _ in range(rng.choice([0, n + m, 3 * (n + m)])):
            a, b = rng.randrange(n + m), rng.randrange(n + m)
            if a != b and a % fam == b % fam:
                edges.append((max(a, b), min(a, b)))
        new = em.new_edges(edges, n)
        assert em.extend_labels(n, m, whole(n, edges, False), new) == whole(n + m, edges, False)
        assert em.extend_reps(n, m, whole(n, edges, True), new) == whole(n + m, edges, True)[n:]
