"""tests/cluster_nearest_model.py (the definition of `mash cluster -B`): the sequential statement against the brute-force one
and the numpy one, on the recorded `mash triangle -E` stdout of the REFERENCE CLI (tests/golden/cluster), on random graphs with
counts and on shapes with a known answer; and the conditions that make the recording a judge of the nearest-representative rule,
asserted on the recorded text alone."""
import inspect
import io
import json
import os
import random
import tokenize

from tests import cluster_greedy_model as gm
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
    for name, text in texts.items():
        e = nm.counted_edges_of_stdout(text, cases["names"])
        want = nm.nearest_brute(n, *columns(e))
        assert nm.nearest(n, *columns(e)) == want, name
        assert nm.nearest_fast(n, *columns(e)) == want, name
        rev = [(c, r, a, b) for r, c, a, b in reversed(e)]                       # neither the order nor the orientation of the edges matters
        assert nm.nearest(n, *columns(rev)) == want, name


def test_three_statements_agree_on_random_graphs():
    rng = random.Random(20261020)
    for _ in range(60):
        n = rng.randint(1, 120)
        m = rng.choice([0, n // 3, n, 3 * n, 8 * n])
        fam = rng.randint(1, 8)
        seen, e = set(), []
        for _ in range(m):
            a, b = rng.randrange(n), rng.randrange(n)
            if a != b and a % fam == b % fam and (max(a, b), min(a, b)) not in seen:
                seen.add((max(a, b), min(a, b)))
                d = rng.choice([0, 1, 3, 16, 32, 64, 64, 64, 1000])               # few denominators and few numerators: ties are common
                e.append((a, b, rng.randint(0, min(d, 4)) * (d // 4 if d >= 4 else 1), d))
        want = nm.nearest_brute(n, *columns(e))
        assert nm.nearest(n, *columns(e)) == want
        assert nm.nearest_fast(n, *columns(e)) == want
        first = gm.reps(n, [x[0] for x in e], [x[1] for x in e])
        assert [i for i in range(n) if want[i] == i] == [i for i in range(n) if first[i] == i]
        pairs = [(x[0], x[1]) for x in e]
        assert gm.no_two_reps_share_an_edge(want, pairs)
        have = {(max(r, c), min(r, c)) for r, c in pairs}
        assert all(want[i] == i or (want[want[i]] == want[i] and (max(i, want[i]), min(i, want[i])) in have) for i in range(n))


def test_shapes_with_a_known_answer():
    # a star around row 7 of 20: rows 0 .. 6 are representatives, 7 joins the best of them -- here row 4, then a tie 2 / 5 goes to 2
    star = [(max(i, 7), min(i, 7), 10 + (i == 4), 64) for i in range(20) if i != 7]
    assert nm.nearest(20, *columns(star)) == [0, 1, 2, 3, 4, 5, 6, 4] + list(range(8, 20))
    star = [(max(i, 7), min(i, 7), 10 + (i in (2, 5)), 64) for i in range(20) if i != 7]
    assert nm.nearest(20, *columns(star)) == [0, 1, 2, 3, 4, 5, 6, 2] + list(range(8, 20))
    # the band of width 3: reps every 4 rows; row 4g + 3 is one step from the LATER representative, three from the earlier one
    n = 61
    band = [(i, i - k, 10 - k, 10) for i in range(n) for k in (1, 2, 3) if i - k >= 0]
    want = [i + 1 if i % 4 == 3 and i + 1 < n else i - i % 4 for i in range(n)]
    assert nm.nearest(n, *columns(band)) == want == nm.nearest_brute(n, *columns(band)) == nm.nearest_fast(n, *columns(band))
    assert want[2] == 0 and want[3] == 4 and want[59] == 60                       # row 2 is a tie (8/10 both sides): the smaller
    # equal fractions under different denominators: 32/64 beside 16/32 -> the smaller representative, whichever carries which
    # (rows 0 and 2 are the representatives, row 1 the member between them); the same for 0/64 beside 0/0
    for e in ([(1, 0, 32, 64), (2, 1, 16, 32)], [(1, 0, 16, 32), (2, 1, 32, 64)], [(1, 0, 0, 64), (2, 1, 0, 0)], [(1, 0, 0, 0), (2, 1, 0, 64)]):
        assert nm.nearest(3, *columns(e)) == [0, 0, 2] == nm.nearest_brute(3, *columns(e))
    assert nm.nearest(3, *columns([(1, 0, 31, 64), (2, 1, 16, 32)])) == [0, 2, 2]
    assert nm.nearest(3, *columns([(1, 0, 0, 64), (2, 1, 1, 1000)])) == [0, 2, 2]
    # a numer == 0 edge as a member's only edge
    assert nm.nearest(2, *columns([(1, 0, 0, 64)])) == [0, 0]
    assert nm.nearest(0, [], [], [], []) == [] and nm.nearest(1, [], [], [], []) == [0] and nm.nearest_fast(0, [], [], [], []) == []


def test_printed_form():
    names = ["a", "b", "c", "d"]
    text = "b\ta\t0\t0\t5/9\nc\tb\t0\t0\t6/9\nd\tc\t0\t0\t1/1\n"                  # the path a - b - c - d; b is nearer to c, a later representative
    assert gm.greedy_stdout_of_triangle(text, names) == "1\t2\ta\n1\t2\tb\n2\t2\tc\n2\t2\td\n"
    assert nm.nearest_stdout_of_triangle(text, names) == "1\t1\ta\ta\n2\t3\tb\tc\n2\t3\tc\tc\n2\t3\td\tc\n"
    assert nm.nearest_stdout_of_triangle(text, names, ["A", "B", "C", "D"]) == "1\t1\tA\tA\n2\t3\tB\tC\n2\t3\tC\tC\n2\t3\tD\tC\n"


def test_no_float_in_the_model():
    """the code of the model (comments and strings apart) has no true division, no float literal and no name with `float` in it"""
    toks = list(tokenize.generate_tokens(io.StringIO(inspect.getsource(nm)).readline))
    assert len(toks) > 500
    for t in toks:
        assert not (t.type == tokenize.OP and t.string in ("/", "/=")), t
        assert not (t.type == tokenize.NAME and "float" in t.string), t
        assert not (t.type == tokenize.NUMBER and not t.string.isdigit()), t


def test_recorded_fixture_is_a_judge_of_the_nearest_rule():
    """on the recorded cases: the representatives are -R's; at least four of the five partitions differ from -R's; dv has a member
    whose representative has a larger index; d2 and v each have a member with an exact tie for best; every denominator is 64"""
    cases, texts = fixture()
    names = cases["names"]
    n = len(names)
    n_reps, moved, later, ties = {}, {}, {}, {}
    for name, text in texts.items():
        e = nm.counted_edges_of_stdout(text, names)
        assert {x[3] for x in e} == {64}, name
        rep = nm.nearest(n, *columns(e))
        first = gm.reps(n, [x[0] for x in e], [x[1] for x in e])
        assert [i for i in range(n) if rep[i] == i] == [i for i in range(n) if first[i] == i], name
        pairs = [(x[0], x[1]) for x in e]
        assert gm.no_two_reps_share_an_edge(rep, pairs), name
        have = {(max(r, c), min(r, c)) for r, c in pairs}
        assert all(rep[i] == i or (max(i, rep[i]), min(i, rep[i])) in have for i in range(n)), name
        n_reps[name] = len(set(rep))
        moved[name] = sum(rep[i] != first[i] for i in range(n))
        later[name] = sum(rep[i] > i for i in range(n))
        ties[name] = len(nm.members_with_a_tie_for_best(rep, e))
    assert n_reps == {"d1": 31, "d2": 22, "d3": 8, "v": 6, "dv": 8}
    assert moved == {"d1": 1, "d2": 5, "d3": 0, "v": 22, "dv": 18}
    assert later == {"d1": 0, "d2": 0, "d3": 0, "v": 0, "dv": 2}
    assert ties == {"d1": 0, "d2": 1, "d3": 0, "v": 1, "dv": 0}
    assert sum(1 for k in moved if moved[k]) >= 4 and later["dv"] >= 1 and ties["d2"] >= 1 and ties["v"] >= 1
