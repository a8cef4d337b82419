"""tests/spectrum_model.py on the recorded stdout of the reference CLI (tests/golden/knn, topk): the running sum at a distance is the
number of lines the reference printed with -d at that distance -- which the recordings with -d 0.08 confirm as they are --, the
counts sum to the lines, and the order on hand-made lines with mixed denominators and 0/0."""
import os

from tests import spectrum_model as sm

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def lines(*path):
    return open(os.path.join(GOLD, *path)).read().splitlines()


def at_or_below(spectrum, d_max):
    """the running sum at the last bin whose printed distance is <= d_max"""
    return max([below for d, _, _, _, below in spectrum if float(d) <= d_max], default=0)


def test_running_sum_is_the_line_count_of_the_thresholded_recording():
    tri = sm.spectrum_of_lines(lines("knn", "triangle.out"))
    assert at_or_below(tri, 0.08) == 189 == len(lines("knn", "triangle_d.out"))
    dist = sm.spectrum_of_lines(lines("topk", "dist.out"))
    assert at_or_below(dist, 0.08) == 418 == len(lines("topk", "dist_d.out"))


def test_bins_and_sums_of_the_recordings():
    tri = sm.spectrum_of_lines(lines("knn", "triangle.out"))
    dist = sm.spectrum_of_lines(lines("topk", "dist.out"))
    assert len(tri) == 54 and len(dist) == 54
    assert sum(x[3] for x in tri) == 903 == tri[-1][4] and sum(x[3] for x in dist) == 1720 == dist[-1][4]
    for sp in (tri, dist):
        assert [float(x[0]) for x in sp] == sorted(float(x[0]) for x in sp)             # ascending distance
        assert all(a[1] * b[2] > b[1] * a[2] for a, b in zip(sp, sp[1:]))                 # one denominator: strictly descending fractions
        assert all(b[4] - a[4] == b[3] for a, b in zip(sp, sp[1:])) and sp[0][4] == sp[0][3]
    assert dist[0][:3] == ("0", 64, 64) and tri[-1][:3] == ("1", 0, 64)


def test_thresholded_recordings_are_prefixes():
    """the spectrum of a -d recording is the head of the unfiltered one: the same bins with the same counts"""
    for full, cut in ((("knn", "triangle.out"), ("knn", "triangle_d.out")), (("topk", "dist.out"), ("topk", "dist_d.out"))):
        a, b = sm.spectrum_of_lines(lines(*full)), sm.spectrum_of_lines(lines(*cut))
        assert 0 < len(b) < len(a) and a[:len(b)] == b


def test_stdout_form():
    text = sm.spectrum_stdout(open(os.path.join(GOLD, "knn", "triangle_d.out")).read())
    rows = text.splitlines()
    assert text.endswith("\n") and all(len(r.split("\t")) == 4 for r in rows)
    assert rows[-1].split("\t")[3] == "189"
    assert sm.spectrum_stdout("") == ""


def line(d, n, m):
    return f"a\tb\t{d}\t0\t{n}/{m}"


def test_order_with_mixed_denominators_and_empty_sketches():
    made = [line("1", 0, 64), line("0.5", 1, 2), line("0.5", 2, 4), line("0", 0, 0), line("0", 64, 64), line("0", 3, 3), line("0.4", 21, 32),
            line("1", 0, 7), line("0.5", 32, 64), line("0.45", 40, 63), line("0.5", 1, 2), line("1", 0, 64)]
    got = [(n, m, c, below) for _, n, m, c, below in sm.spectrum_of_lines(made)]
    assert got == [(0, 0, 1, 1), (3, 3, 1, 2), (64, 64, 1, 3),                     # 0/0 orders as 1/1, equal fractions by ascending denominator
                   (21, 32, 1, 4), (40, 63, 1, 5),                                   # 21/32 = 0.656 before 40/63 = 0.635
                   (1, 2, 2, 7), (2, 4, 1, 8), (32, 64, 1, 9),                       # one half three times over, two lines in the first
                   (0, 7, 1, 10), (0, 64, 2, 12)]
    assert sm.before((0, 0), (1, 1)) == -1 and sm.before((1, 1), (0, 0)) == 1 and sm.before((5, 9), (5, 9)) == 0
    assert sm.before((0xFFFFFFFE, 0xFFFFFFFF), (0xFFFFFFFD, 0xFFFFFFFE)) == -1      # exact beyond what a double tells apart


def test_spectrum_of_counts_agrees_with_the_lines():
    import numpy as np
    made = [line("1", 0, 64), line("0.5", 1, 2), line("0", 0, 0), line("0.5", 1, 2), line("0", 64, 64)]
    numer, denom, count = sm.spectrum_of_counts(np.array([0, 1, 0, 1, 64]), np.array([64, 2, 0, 2, 64]))
    assert [(int(a), int(b), int(c)) for a, b, c in zip(numer, denom, count)] == [(n, m, c) for _, n, m, c, _ in sm.spectrum_of_lines(made)]
