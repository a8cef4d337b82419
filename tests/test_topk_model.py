"""tests/topk_model.py (the definition of `mash dist -N`) against an independent sorted() over fractions.Fraction, and over
recorded stdout of the reference CLI (tests/golden/cli, read only)."""
import os
import random
from fractions import Fraction

import pytest

from tests import topk_model as tm

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cli")


def by_fractions(numer, denom, passed, k):
    idx = [r for r in range(len(numer)) if passed[r]]
    return sorted(idx, key=lambda r: (-Fraction(numer[r], denom[r] or 1), r))[:k]


def test_near_equal_fractions_are_told_apart():
    """the pairs a float32 key merges: 4999/9999 < 5000/10001 < 5000/10000, and tenfold"""
    import numpy as np
    for numer, denom in (([4999, 5000, 5000], [9999, 10001, 10000]), ([49999, 50000, 50000], [99999, 100001, 100000])):
        assert np.float32(numer[0]) / np.float32(denom[0]) == np.float32(numer[1]) / np.float32(denom[1])      # (the hazard is real)
        assert tm.rank_row(numer, denom, None, 3) == [2, 1, 0]
        assert tm.rank_row(numer, denom, None, 2) == [2, 1]
        assert tm.rank_row(numer, denom, [1, 1, 0], 2) == [1, 0]


def test_zero_numerators_tie_in_index_order():
    numer, denom = [0, 0, 1, 0, 0], [7, 0, 1000, 3, 0]
    assert tm.rank_row(numer, denom, None, 5) == [2, 0, 1, 3, 4]
    assert tm.rank_row(numer, denom, [1, 1, 0, 1, 1], 2) == [0, 1]


def test_model_against_fractions_on_random_tables():
    rng = random.Random(20261017)
    for t in range(300):
        s = rng.choice([1, 4, 64, 1000, 100002])
        nref = rng.randrange(1, 60)
        denom = [s if rng.random() < 0.7 else rng.randrange(0, s + 1) for _ in range(nref)]
        numer = [0 if rng.random() < 0.3 else rng.randrange(0, d + 1) for d in denom]
        if t % 5 == 0:                                           # equal fractions spelled differently
            for r in range(0, nref - 1, 2):
                m = rng.randrange(1, 4)
                numer[r + 1], denom[r + 1] = numer[r] * m, denom[r] * m
        passed = [rng.random() < 0.8 for _ in range(nref)]
        for k in (1, 3, 10, 1000):
            assert tm.rank_row(numer, denom, passed, k) == by_fractions(numer, denom, passed, k)
    assert tm.topk([[1, 2], [0, 0]], [[2, 2], [5, 0]], None, 1) == [[1], [0]]


@pytest.mark.parametrize("name", ["dist_individual", "x_dist_protein", "dist_self", "dist_maxd"])
def test_model_over_recorded_reference_stdout(name):
    text = open(os.path.join(GOLD, name + ".out")).read()
    runs = tm.query_runs(text)
    assert runs and sum(len(l) for _, l in runs) == len(text.splitlines())
    assert len({q for q, _ in runs}) == len(runs)               # every query is one run
    for k in (1, 2, 3, 1000):
        got = tm.query_runs(tm.topk_of_stdout(text, k))
        assert [q for q, _ in got] == [q for q, _ in runs]
        for (_, lines), (_, all_lines) in zip(got, runs):
            assert len(lines) == min(k, len(all_lines))
            fr = [Fraction(x, y or 1) for x, y in map(tm.fraction_of_line, lines)]
            assert fr == sorted(fr, reverse=True) and fr[0] == max(Fraction(x, y or 1) for x, y in map(tm.fraction_of_line, all_lines))
            at = [all_lines.index(ln) for ln in lines]
            assert len(set(at)) == len(at)                      # every line is one of the query's own, none twice
            for i in range(len(at) - 1):
                assert fr[i] > fr[i + 1] or at[i] < at[i + 1]   # equal fractions in reference order
            if k >= len(all_lines):
                assert sorted(lines) == sorted(all_lines)
    if name == "dist_self":                                      # a sketch is its own nearest reference
        for q, lines in tm.query_runs(tm.topk_of_stdout(text, 1)):
            assert lines[0].split("\t")[0] == q


def test_fast_ranking_of_long_rows_is_the_same_ranking():
    """rank_row_fast (what the GPU test runs on rows of 20 000 references) against rank_row"""
    import numpy as np
    rng = random.Random(7)
    for _ in range(120):
        n, s = rng.randrange(1, 3000), rng.choice([8, 1000, 100002])
        denom = [s if rng.random() < 0.7 else rng.randrange(0, s + 1) for _ in range(n)]
        zero = rng.choice([0.2, 0.99])
        numer = [0 if rng.random() < zero else rng.randrange(0, d + 1) for d in denom]
        passed = [rng.random() < 0.8 for _ in range(n)]
        for k in (1, 10, 100, 1024):
            assert tm.rank_row_fast(np.array(numer), np.array(denom), np.array(passed), k) == tm.rank_row(numer, denom, passed, k)
            assert tm.rank_row_fast(np.array(numer), np.array(denom), None, k) == tm.rank_row(numer, denom, None, k)
