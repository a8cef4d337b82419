"""tests/within_model.py -- the statement of `mash within` the device tests compare against -- checked on the CPU: its closed
form against its serial walk (containSketches, CommandContain.cpp:231-263) on random and adversarial lists, the conversion of
-e into a smallest passing j at exact boundaries, and, through sketches of the fixture made by the CPU oracle, against every
recording of the reference CLI in tests/golden/within byte for byte.  The conditions tests/golden/make_within_golden.py chose
the fixture's seed by are asserted again, on the recorded text and under the model."""
import math
import random
import struct

import pytest

from tests import within_fixture as wf
from tests import within_model as wm


def both(ref, qry):
    a, b = wm.walk(ref, qry), wm.closed(ref, qry)
    assert a == b, (ref, qry, a, b)
    return a


def test_closed_form_equals_the_walk_on_random_lists():
    rng = random.Random(20261021)
    for _ in range(20000):
        u = rng.randint(2, 39)
        ref = sorted(rng.sample(range(u), rng.randint(0, min(12, u))))
        qry = sorted(rng.sample(range(u), rng.randint(0, min(12, u))))
        both(ref, qry)


def test_closed_form_equals_the_walk_on_large_values():
    rng = random.Random(7)
    for _ in range(300):
        pool = [rng.getrandbits(64) for _ in range(400)] + [2 ** 64 - 1, 0]
        ref = sorted(set(rng.sample(pool, rng.randint(1, 300))))
        qry = sorted(set(rng.sample(pool, rng.randint(1, 300))))
        both(ref, qry)


def test_adversarial_lists():
    assert both([], []) == (0, 0)
    assert both([], [1, 2, 3]) == (0, 0)
    assert both([1, 2, 3], []) == (0, 0)
    # max(R) shared: the equal step consumes the query's hash too (the comparison is <=)
    assert both([1, 5, 9], [2, 9, 11, 12]) == (1, 2)
    # max(R) not shared: the walk stops in front of the first larger query hash
    assert both([1, 5, 9], [2, 10, 11, 12]) == (0, 1)
    # a shared hash at query rank j (counted) and at rank j + 1 (not reached): j = |R| = 2
    assert both([3, 7], [1, 7, 8]) == (1, 2)
    assert both([3, 8], [1, 2, 8]) == (0, 2)
    assert both([2, 8], [1, 2, 8, 9]) == (1, 2)
    # disjoint ranges, both orders: the reference below the query gives j = 0, above it j = min(|R|, |Q|) and nothing common
    assert both([1, 2, 3], [10, 11]) == (0, 0)
    assert both([10, 11, 12], [1, 2]) == (0, 2)
    assert both([10, 11], [1, 2, 3]) == (0, 2)
    # identical lists
    assert both(list(range(5, 50, 3)), list(range(5, 50, 3))) == (15, 15)
    # one element each
    assert both([4], [4]) == (1, 1)
    assert both([4], [5]) == (0, 0)
    assert both([5], [4]) == (0, 1)


def test_terminations_are_told_apart():
    assert wm.termination([1, 2, 3, 40], [2, 3]) == "Q"
    assert wm.termination([1, 40], [2, 3, 4]) == "R"
    assert wm.termination([1, 2, 3], [2, 30, 40]) == "exhausted"
    assert wm.termination([], [1]) == "empty"


def f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def test_j_min_at_exact_boundaries():
    # (float)0.05 lies above 0.05 = 1 / sqrt(400), so j = 400 passes and 399 does not
    assert f32(0.05) > 0.05 and wm.j_min(f32(0.05)) == 400
    assert wm.passes(400, f32(0.05)) and not wm.passes(399, f32(0.05))
    # the double 0.05 is below 1 / sqrt(400) = 0.05000000000000000277: the float conversion decides this pair
    assert 1.0 / math.sqrt(400) > 0 and (wm.j_min(0.05) == 400) == (1.0 / math.sqrt(400) <= 0.05)
    # (float)0.1 lies above 0.1 = 1 / sqrt(100)
    assert f32(0.1) > 0.1 and wm.j_min(f32(0.1)) == 100
    # (float)0.7 lies BELOW 0.7; 1 / sqrt(2) = 0.7071 is above both, 1 / sqrt(3) = 0.577 below both
    assert f32(0.7) < 0.7 and wm.j_min(f32(0.7)) == 3 and wm.j_min(0.7) == 3
    # a float below its double with a j in between: e = 1 / sqrt(j) as a double passes j, its float (rounded down) does not
    hit = 0
    for j in range(2, 2000):
        e = 1.0 / math.sqrt(j)
        if f32(e) < e:
            assert wm.j_min(e) == j and wm.j_min(f32(e)) == j + 1
            hit += 1
    assert hit > 100
    assert wm.j_min(1.0) == 1 and wm.j_min(2.5) == 1 and wm.j_min(math.inf) == 1
    assert wm.j_min(0.0) is None and wm.j_min(-1.0) is None and wm.j_min(math.nan) is None
    for e in (0.9999, 0.5, 0.3, 0.011, 1e-3):
        j = wm.j_min(e)
        assert wm.passes(j, e) and (j == 1 or not wm.passes(j - 1, e))


def test_line_format_is_the_default_ostream_format():
    assert wm.line(0, 1, "r", "q") == "0\t1\tr\tq\n"
    assert wm.line(1000, 1000, "r", "q") == "1\t0.0316228\tr\tq\n"
    assert wm.line(4, 85, "a b", "c") == "0.0470588\t0.108465\ta b\tc\n"


META = wf.load_cases()


@pytest.mark.parametrize("case", META["cases"], ids=[c["name"] for c in META["cases"]])
def test_model_reproduces_the_recorded_output(case):
    assert wf.model_stdout(case, META) == wf.recorded(case["name"])
    assert case["exit"] == (1 if case["name"].startswith("refuses") else 0)


def test_fixture_conditions_on_the_text():
    e005, e03, e1 = (wm.parse(wf.recorded(n)) for n in ("fa_e005", "fa_e03", "fa_e1"))
    scores = {float(l[0]) for l in e1}
    assert 0.0 in scores and 1.0 in scores and any(0 < x < 1 for x in scores)
    nref, nqry = 4, 8
    assert len(e1) < nref * nqry                                           # some pair is absent even under -e 1: j = 0
    pairs = lambda ls: {(l[2], l[3]) for l in ls}
    assert pairs(e005) and pairs(e005) < pairs(e03) < pairs(e1)              # some pair passes one threshold and not the next
    assert wf.recorded("quirk_a_continues") == wf.recorded("fa_e1") == wf.recorded("quirk_z_continues")
    assert wf.recorded("refuses_k") == "" and wf.recorded("refuses_n") == ""


def test_fixture_covers_all_three_terminations():
    seen = set()
    for name in ("fa_e1", "fa_s200_e1_p3"):
        refs, queries, _, _ = wf.case_inputs(next(c for c in META["cases"] if c["name"] == name), META)
        seen |= {wm.termination(r, q) for _, r in refs for _, q in queries}
    assert {"Q", "R", "exhausted"} <= seen
    # ... and the pairs absent under -e 1 are the model's j = 0
    refs, queries, _, _ = wf.case_inputs(next(c for c in META["cases"] if c["name"] == "fa_e1"), META)
    absent = {(rn, qn) for rn, r in refs for qn, q in queries if wm.closed(r, q)[1] == 0}
    printed = {(l[2], l[3]) for l in wm.parse(wf.recorded("fa_e1"))}
    assert absent and not absent & printed and len(absent) + len(printed) == len(refs) * len(queries)
