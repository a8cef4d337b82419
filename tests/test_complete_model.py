"""tests/complete_model.py against itself: the sequential walk of the definition, the mutual-link rounds (the statement the device
implements) and the adjacency form agree -- on the labels, and the first two on the SET of merges -- over random tie-heavy graphs
(2 .. 14 rows, 1 .. 8 fraction values under one and under three denominators) and over the five recorded cases of
tests/golden/cluster.  Every cluster is a clique, no two final clusters are linked, the recorded cases give 33 / 24 / 9 / 7 / 8
clusters and differ from the single-linkage partition, a clique of equal fractions takes n - 1 rounds, and the key the adjacency
form orders by orders as the fraction does."""
import json
import os
import random
from fractions import Fraction

import pytest

from tests import cluster_model as cm
from tests import complete_model as lm
from tests import forest_model as fm

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cluster")
COUNTS = {"d1": 33, "d2": 24, "d3": 9, "v": 7, "dv": 8}
ROUNDS = {"d1": 4, "d2": 7, "d3": 9, "v": 10, "dv": 9}              # rounds of mutual links that merged something


def random_graph(rng, denoms):
    n = rng.randint(2, 14)
    values = rng.randint(1, 8)
    p = rng.choice((0.3, 0.6, 0.9, 1.0))
    edges = []
    for r in range(1, n):
        for c in range(r):
            if rng.random() < p:
                d = rng.choice(denoms)
                edges.append((r, c, rng.randint(1, values) * (d // 8), d))
    rng.shuffle(edges)
    return n, edges


def check(n, edges):
    lab, merges = lm.walk(n, edges)
    lab_r, merges_r, count = lm.rounds(n, edges)
    assert lab_r == lab and merges_r == set(merges) and len(merges_r) == len(merges)
    assert lm.labels(n, edges) == lab
    assert lm.not_cliques(lab, edges) == [] and lm.linked_pairs(lab, edges) == []
    assert all(lab[lab[i]] == lab[i] <= i for i in range(n))
    assert (count == 0) == (not edges) and count <= max(n - 1, 0)
    return lab, count


@pytest.mark.parametrize("denoms", [(64,), (16, 32, 64)], ids=["one denominator", "three denominators"])
def test_three_forms_agree_on_random_tie_heavy_graphs(denoms):
    rng = random.Random(20261021 + len(denoms))
    for _ in range(750):
        check(*random_graph(rng, denoms))


def recorded():
    cases = json.load(open(os.path.join(GOLD, "cases.json")))
    return cases, {c["name"]: open(os.path.join(GOLD, c["name"] + ".out")).read() for c in cases["cases"]}


@pytest.mark.parametrize("name", sorted(COUNTS))
def test_recorded_cases(name):
    cases, texts = recorded()
    names = cases["names"]
    edges = [e[:4] for e in fm.lines_of_stdout(texts[name], names)]
    lab, count = check(len(names), edges)
    assert len(set(lab)) == COUNTS[name] and count == ROUNDS[name]
    single = cm.labels(len(names), [e[0] for e in edges], [e[1] for e in edges])
    assert lab != single and len(set(single)) < len(set(lab))
    assert all(single[i] == single[lab[i]] for i in range(len(names)))          # a refinement of the single-linkage partition
    text = lm.complete_stdout_of_triangle(texts[name], names)
    assert text == cm.cluster_stdout(lab, names) and text != cm.cluster_stdout_of_triangle(texts[name], names)
    assert lm.complete_stdout_of_triangle(texts[name], names, cases["comments"]) == cm.cluster_stdout(lab, cases["comments"])


def test_the_partition_does_not_depend_on_the_order_of_the_edges():
    rng = random.Random(7)
    for _ in range(50):
        n, edges = random_graph(rng, (16, 32, 64))
        want = lm.labels(n, edges)
        again = [(e[1], e[0], e[2], e[3]) if rng.random() < 0.5 else e for e in edges]
        rng.shuffle(again)
        assert lm.labels(n, again) == want and lm.walk(n, again)[0] == want


def test_small_cases_by_hand():
    half = [(r, c, 1, 2) for r in range(1, 6) for c in range(r)]
    assert check(6, half) == ([0] * 6, 5)                                          # equal fractions: one pair per round
    # the same without {5, 0}: the cliques {0 .. 4} and {1 .. 5} overlap; (1, 0) is the first link, so 0's side wins and 5 stays alone
    assert check(6, [e for e in half if (e[0], e[1]) != (5, 0)])[0] == [0, 0, 0, 0, 0, 5]
    # a path: pairs, never triples; with equal fractions 2 prefers (2, 1), so (3, 2) is mutual only in the second round
    assert check(5, [(i, i - 1, 1, 2) for i in range(1, 5)]) == ([0, 0, 2, 2, 4], 2)
    # the better edge first, whatever the rows: (2, 1) at 3/4 beats (1, 0) at 1/2
    assert check(3, [(1, 0, 1, 2), (2, 1, 3, 4)])[0] == [0, 1, 1]
    # 0/0 counts as 0/1 and ties with 0/5
    assert check(3, [(1, 0, 0, 0), (2, 0, 0, 5)])[0] == [0, 0, 2]
    # both ends of a surviving link merge in one round, and one of the four pairs is missing: {0, 1} and {2, 3} stay apart
    four = [(1, 0, 7, 8), (3, 2, 7, 8), (2, 0, 1, 2), (3, 0, 1, 2), (2, 1, 1, 2)]
    assert check(4, four) == ([0, 0, 2, 2], 1)
    assert check(4, four + [(3, 1, 1, 4)]) == ([0, 0, 0, 0], 2)


def test_key_orders_as_the_fraction():
    rng = random.Random(3)
    top = fm.DENOM_LIMIT - 1
    pairs = [(rng.randint(0, d), d) for d in (1, 2, 3, 64, 1000, top - 1, top) for _ in range(40)] + [(0, 0), (top - 1, top), (top - 2, top - 1)]
    for a in pairs:
        for b in pairs:
            fa, fb = fm.fraction(*a), fm.fraction(*b)
            ka, kb = fm.key(*a), fm.key(*b)
            assert (ka < kb) == (fa < fb) and (ka == kb) == (fa == fb)
            # ... and so do the links' sort keys built on either
            assert (lm.link_key(ka, 5, 2) < lm.link_key(kb, 5, 2)) == (lm.link_key(fa, 5, 2) < lm.link_key(fb, 5, 2))
    assert lm.link_key(Fraction(1, 2), 3, 9) == lm.link_key(Fraction(2, 4), 9, 3) < lm.link_key(Fraction(1, 2), 9, 4)
