"""tests/cluster_medoid_model.py (the definition of `mash cluster -M`): the sequential statement against the brute-force one and
the numpy one, on the recorded `mash triangle -E` stdout of the REFERENCE CLI (tests/golden/cluster), on random graphs with
counts and on shapes with a known answer; the conditions that make the recording a judge of the medoid rule, asserted on the
recorded text alone; and the printed form, whose first three fields are `mash cluster`'s."""
import inspect
import io
import json
import os
import random
import tokenize

from tests import cluster_medoid_model as mm
from tests import cluster_model as cm
from tests import cluster_nearest_model as nm

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cluster")


def fixture():
    cases = json.load(open(os.path.join(GOLD, "cases.json")))
    texts = {c["name"]: open(os.path.join(GOLD, c["name"] + ".out")).read() for c in cases["cases"]}
    return cases, texts


def columns(e):
    return [[x[k] for x in e] for k in range(4)]


def test_three_statements_agree_on_the_fixture():
    cases, texts = fixture()
    n = len(cases["names"])
    assert sorted(texts) == ["d1", "d2", "d3", "dv", "v"]
    for name, text in texts.items():
        e = nm.counted_edges_of_stdout(text, cases["names"])
        want = mm.medoid_brute(n, *columns(e))
        assert mm.medoid(n, *columns(e)) == want, name
        assert mm.medoid_fast(n, *columns(e)) == want, name
        rev = [(c, r, a, b) for r, c, a, b in reversed(e)]                       # neither the order nor the orientation of the edges matters
        assert mm.medoid(n, *columns(rev)) == want, name
        assert want[0] == cm.labels(n, [x[0] for x in e], [x[1] for x in e]), name


def test_three_statements_agree_on_random_graphs():
    rng = random.Random(20261020)
    moved = ties = 0
    for _ in range(60):
        n = rng.randint(1, 120)
        m = rng.choice([0, n // 3, n, 3 * n, 8 * n])
        fam = rng.randint(1, 8)
        seen, e = set(), []
        for _ in range(m):
            a, b = rng.randrange(n), rng.randrange(n)
            if a != b and a % fam == b % fam and (max(a, b), min(a, b)) not in seen:
                seen.add((max(a, b), min(a, b)))
                d = rng.choice([0, 1, 3, 16, 32, 63, 64, 64, 64, 1000])           # few denominators and few numerators: ties are common
                e.append((a, b, rng.randint(0, min(d, 4)) * (d // 4 if d >= 4 else 1), d))
        lab, med, score = want = mm.medoid_brute(n, *columns(e))
        assert mm.medoid(n, *columns(e)) == want
        assert mm.medoid_fast(n, *columns(e)) == want
        assert sum(score) == 2 * sum(mm.weight(a, b) for _, _, a, b in e)         # every edge counts at both its ends
        for i in range(n):
            assert lab[med[i]] == lab[i] and med[med[i]] == med[i] and score[med[i]] >= score[i]
            assert med[i] <= i or score[med[i]] > score[i]
        moved += bool(mm.clusters_with_another_medoid(lab, med))
        ties += bool(mm.clusters_with_a_tie(lab, score))
    assert moved >= 20 and ties >= 20                                             # the graphs do tell the medoid from the first member


def test_shapes_with_a_known_answer():
    one = mm.ONE
    # a star whose centre is the LAST row
    star = [(19, i, 32, 64) for i in range(19)]
    assert mm.medoid(20, *columns(star)) == ([0] * 20, [19] * 20, [one // 2] * 19 + [19 * (one // 2)])
    # a clique of equal weights: every score equal, the smallest row
    clique = [(i, j, 16, 64) for i in range(6) for j in range(i)]
    assert mm.medoid(6, *columns(clique)) == ([0] * 6, [0] * 6, [5 * (one // 4)] * 6)
    # a path of five rows: the inner rows tie at two edges each, the smallest of them wins
    path = [(i, i - 1, 64, 64) for i in range(1, 5)]
    assert mm.medoid(5, *columns(path)) == ([0] * 5, [1] * 5, [one, 2 * one, 2 * one, 2 * one, one])
    # two clusters interleaved in index order: the even rows around row 4, the odd rows around row 3
    two = [(4, 0, 10, 64), (4, 2, 10, 64), (6, 4, 10, 64), (3, 1, 10, 64), (5, 3, 10, 64)]
    lab, med, _ = mm.medoid(7, *columns(two))
    assert lab == [0, 1, 0, 1, 0, 1, 0] and med == [4, 3, 4, 3, 4, 3, 4]
    # mixed denominators: 21/63 is no multiple of 2^-32, its floor is taken per edge, before the sum
    assert mm.weight(21, 63) == one // 3 == 1431655765 and 3 * mm.weight(21, 63) == one - 1
    assert mm.weight(32, 64) == mm.weight(16, 32) == one // 2 and mm.weight(0, 0) == 0 == mm.weight(0, 64) and mm.weight(64, 64) == one
    e = [(1, 0, 21, 63), (2, 1, 21, 63), (3, 2, 21, 63), (3, 0, 32, 64)]
    assert mm.medoid(4, *columns(e))[2] == [one // 3 + one // 2, 2 * (one // 3), 2 * (one // 3), one // 3 + one // 2]
    assert mm.medoid(4, *columns(e))[1] == [0] * 4                                # rows 0 and 3 tie: the smaller
    # 0/0 and 0/d edges join clusters and add nothing
    e = [(1, 0, 0, 0), (2, 1, 0, 64), (3, 2, 1, 64)]
    assert mm.medoid(5, *columns(e)) == ([0, 0, 0, 0, 4], [2, 2, 2, 2, 4], [0, 0, one // 64, one // 64, 0]) == mm.medoid_brute(5, *columns(e))
    # a non-edge of the cluster counts 0: row 0 has ONE strong edge, row 2 two weaker ones that sum to more
    e = [(1, 0, 60, 64), (2, 1, 40, 64), (3, 2, 40, 64)]
    assert mm.medoid(4, *columns(e))[1] == [1] * 4
    assert mm.medoid(0, [], [], [], []) == ([], [], []) == mm.medoid_fast(0, [], [], [], [])
    assert mm.medoid(1, [], [], [], []) == ([0], [0], [0]) == mm.medoid_brute(1, [], [], [], []) == mm.medoid_fast(1, [], [], [], [])


def test_printed_form():
    names = ["a", "b", "c", "d", "e"]
    text = "b\ta\t0\t0\t5/9\nc\tb\t0\t0\t6/9\nd\tc\t0\t0\t1/9\n"                  # the path a - b - c - d, and e alone: b has the most
    assert mm.medoid_stdout_of_triangle(text, names) == "1\t4\ta\tb\n1\t4\tb\tb\n1\t4\tc\tb\n1\t4\td\tb\n2\t1\te\te\n"
    assert mm.medoid_stdout_of_triangle(text, names, list("ABCDE")) == "1\t4\tA\tB\n1\t4\tB\tB\n1\t4\tC\tB\n1\t4\tD\tB\n2\t1\tE\tE\n"


def test_fourth_field_cut_off_is_plain_cluster_output():
    cases, texts = fixture()
    names = cases["names"]
    shown = ["comment of " + nm_ for nm_ in names]
    for name, text in texts.items():
        for sh in (None, shown):
            got = mm.medoid_stdout_of_triangle(text, names, sh)
            cut = "".join(ln.rsplit("\t", 1)[0] + "\n" for ln in got.splitlines())
            assert cut == cm.cluster_stdout_of_triangle(text, names, sh), name
            assert all(ln.count("\t") == 3 for ln in got.splitlines()) and len(got.splitlines()) == len(names)


def test_no_float_in_the_model():
    """the code of the model (comments and strings apart) has no true division, no float literal and no name with `float` in it"""
    toks = list(tokenize.generate_tokens(io.StringIO(inspect.getsource(mm)).readline))
    assert len(toks) > 500
    for t in toks:
        assert not (t.type == tokenize.OP and t.string in ("/", "/=")), t
        assert not (t.type == tokenize.NAME and "float" in t.string), t
        assert not (t.type == tokenize.NUMBER and not t.string.isdigit()), t


def test_recorded_fixture_is_a_judge_of_the_medoid_rule():
    """on the recorded cases: how many clusters have a medoid that is not their first member, and how many a tie for the top score"""
    cases, texts = fixture()
    names = cases["names"]
    n = len(names)
    moved, ties = {}, {}
    for name, text in texts.items():
        e = nm.counted_edges_of_stdout(text, names)
        lab, med, score = mm.medoid(n, *columns(e))
        moved[name] = len(mm.clusters_with_another_medoid(lab, med))
        ties[name] = len(mm.clusters_with_a_tie(lab, score))
    assert moved == {"d1": 2, "d2": 3, "d3": 3, "v": 1, "dv": 1}
    assert ties == {"d1": 5, "d2": 3, "d3": 1, "v": 0, "dv": 0}
