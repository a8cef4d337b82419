"""tests/knn_model.py (the definition of `mash triangle -N` the GPU tests compare with) against a brute-force ranking of the
full n x n matrix on small random integer tables, and the conditions the recorded fixture tests/golden/knn has to meet
(tests/golden/make_knn_golden.py asserts the same when it records)."""
import functools
import json
import os

import numpy as np
import pytest

from tests import knn_model as km

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "knn")


def brute(numer, denom, passed, n, k):
    """every ordered pair (i, j), j != i, ranked per row by cross-multiplied Python integers, ties by j"""
    def before(a, b):
        l, r = a[0] * (b[1] or 1), b[0] * (a[1] or 1)
        return -1 if l > r or (l == r and a[2] < b[2]) else 1
    out = []
    for i in range(n):
        row = []
        for j in range(n):
            if j == i:
                continue
            t = km.tri_index(i, j)
            if passed is None or passed[t]:
                row.append((int(numer[t]), int(denom[t]), j))
        row.sort(key=functools.cmp_to_key(before))
        out.append([e[2] for e in row[:k]])
    return out


@pytest.mark.parametrize("seed", range(6))
def test_model_against_brute_force(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 40))
    pairs = n * (n - 1) // 2
    s = int(rng.choice([1, 3, 8, 1000]))
    denom = rng.integers(0, s + 1, pairs)                        # (0/0 occurs: two empty sketches)
    numer = (rng.random(pairs) * (denom + 1)).astype(np.int64)
    numer[rng.random(pairs) < 0.3] = 0
    for passed in (None, rng.random(pairs) < 0.5, np.zeros(pairs, dtype=bool)):
        for k in (1, 2, 5, n - 1, n + 3):
            assert km.knn_of_pairs(numer, denom, passed, n, k) == brute(numer, denom, passed, n, k), (n, s, k)


def test_both_ranking_paths_of_the_model_agree():
    """below 2^26 the model ranks by correctly rounded quotients, above by cross-multiplied integers: the same values scaled by
    2^26 (numer and denom alike, so every fraction keeps its value) take the other path and must give the same lists"""
    rng = np.random.default_rng(99)
    n = 30
    pairs = n * (n - 1) // 2
    denom = rng.integers(1, 9, pairs)
    numer = (rng.random(pairs) * (denom + 1)).astype(np.int64)
    passed = rng.random(pairs) < 0.7
    scale = rng.choice([1, 2, 3], pairs)                          # (equal fractions spelled differently)
    small = km.knn_of_pairs(numer * scale, denom * scale, passed, n, 7)
    assert small == km.knn_of_pairs(numer * scale << 26, denom * scale << 26, passed, n, 7) == brute(numer, denom, passed, n, 7)


def test_all_equal_fractions_give_index_order_across_the_diagonal():
    n = 9
    pairs = n * (n - 1) // 2
    got = km.knn_of_pairs(np.full(pairs, 3), np.full(pairs, 7), None, n, 4)
    assert got == [[j for j in range(n) if j != i][:4] for i in range(n)]


def test_stdout_form_gives_both_rows_an_entry():
    names = ["a", "b", "c"]
    stdout = "b\ta\t0.1\t0\t5/8\nc\ta\t1\t1\t0/8\nc\tb\t0.1\t0\t10/16\n"
    assert km.knn_of_stdout(stdout, names, 1) == "a\tb\t0.1\t0\t5/8\nb\ta\t0.1\t0\t5/8\nc\tb\t0.1\t0\t10/16\n"
    assert km.knn_of_stdout(stdout, names, 5).splitlines()[:2] == ["a\tb\t0.1\t0\t5/8", "a\tc\t1\t1\t0/8"]
    assert km.has_tie_across_diagonal(stdout, names)             # b: a (below) and c (above) at 5/8 = 10/16
    assert km.has_tie_across_cut(stdout, names, 1) and not km.has_tie_across_cut(stdout, names, 2)


def test_recorded_fixture_meets_its_conditions():
    cases = json.load(open(os.path.join(GOLD, "cases.json")))
    names = cases["names"]
    read = lambda n: open(os.path.join(GOLD, n + ".out")).read()
    plain, with_d, with_v = read("triangle"), read("triangle_d"), read("triangle_v")
    assert len(names) == cases["sketches"] == 43 and len(plain.splitlines()) == 43 * 42 // 2
    for n in cases["ns"]:
        assert km.has_tie_across_cut(plain, names, n), n
    assert km.has_tie_across_diagonal(plain, names)
    lines = [len(r) for r in km.entries_of_stdout(with_d, names)]
    assert any(x == 0 for x in lines) and any(0 < x < 3 for x in lines) and any(3 <= x < 10 for x in lines) and any(x >= 10 for x in lines)
    assert 0 < len(with_v.splitlines()) < len(plain.splitlines())
    assert set(with_d.splitlines()) < set(plain.splitlines()) and set(with_v.splitlines()) < set(plain.splitlines())
