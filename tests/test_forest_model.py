"""tests/forest_model.py (the definition of `mash cluster -T`) against its brute-force second statement on random graphs with heavy
ties and mixed denominators; the conditions that make the recorded fixture tests/golden/cluster decisive for the forest, re-asserted
on the recorded text alone; the cut property against tests/cluster_model.py; and the lemma behind the 64-bit weight key of
mash_amd/csrc/forest_key.h -- exhaustively for denominators up to 128, on seeded random pairs up to 2^21 - 1, and through a
stand-alone C++ program that includes the header itself."""
import json
import os
import random
import subprocess
from fractions import Fraction

import numpy as np

from tests import cluster_model as cm
from tests import forest_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "cluster")
SIZES = {"d1": 15, "d2": 28, "d3": 37, "v": 39, "dv": 39}
CLUSTERS = {"d1": 29, "d2": 16, "d3": 7, "v": 5, "dv": 5}


def fixture():
    cases = json.load(open(os.path.join(GOLD, "cases.json")))
    texts = {c["name"]: open(os.path.join(GOLD, c["name"] + ".out")).read() for c in cases["cases"]}
    return cases, texts


def random_graph(rng, n, m, denoms, fam):
    have = set()
    out = []
    for _ in range(m):
        a, b = rng.randrange(n), rng.randrange(n)
        if a == b or a % fam != b % fam or (max(a, b), min(a, b)) in have:
            continue
        have.add((max(a, b), min(a, b)))
        d = rng.choice(denoms)
        out.append((max(a, b), min(a, b), rng.randint(0 if d == 0 else 1, d) if d else 0, d))
    return out


def test_model_against_the_brute_force_statement():
    rng = random.Random(20261019)
    for trial in range(40):
        n = rng.randint(2, 60)
        denoms = rng.choice([[4], [2, 4, 64], [3, 5, 6, 10, 12], [64], [0, 1, 2]])      # heavy ties, equal fractions under several denominators
        e = random_graph(rng, n, rng.choice([n // 2, n, 3 * n, 8 * n]), denoms, rng.randint(1, 3))
        rng.shuffle(e)
        want = fm.forest_brute(n, e)
        assert fm.forest(n, e) == want, trial
        got = fm.forest_fast(n, *[[x[i] for x in e] for i in range(4)])
        assert [e[i] for i in got] == want, trial
        assert all(fm.before(a, b) and not fm.before(b, a) for a, b in zip(want, want[1:]))
        lab = cm.labels(n, [x[0] for x in e], [x[1] for x in e])
        assert len(want) == n - len(set(lab))


def test_numpy_form_on_a_large_tied_graph():
    rng = np.random.default_rng(7)
    n, m = 3000, 400000
    row = rng.integers(1, n, m)
    col = (rng.random(m) * row).astype(np.int64)
    pair = np.unique(row << 32 | col)
    row, col = pair >> 32, pair & 0xFFFFFFFF
    denom = rng.choice([500, 1000, 250], len(row))
    numer = (rng.integers(1, 50, len(row)) * denom) // 50              # fifty fraction values, each under three denominators
    e = list(zip(row.tolist(), col.tolist(), numer.tolist(), denom.tolist()))
    got = fm.forest_fast(n, row, col, numer, denom)
    assert [e[i] for i in got] == fm.forest(n, e)


def test_recorded_fixture_is_decisive_for_the_forest():
    cases, texts = fixture()
    names = cases["names"]
    n = len(names)
    forests = {}
    for name, text in texts.items():
        lines = fm.lines_of_stdout(text, names)
        assert all(r > c for r, c, _, _, _ in lines) and [(l[0], l[1]) for l in lines] == sorted((l[0], l[1]) for l in lines), name
        assert all(l[3] == 64 for l in lines), name                    # (every recorded denominator is 64: mixed ones are synthetic)
        f = fm.forest_lines(text, names)
        forests[name] = f
        assert f == fm.forest(n, lines) == fm.forest_brute(n, lines), name           # the stable sort IS the order
        assert len(f) == SIZES[name] == n - CLUSTERS[name], name
        lab = cm.labels(n, [l[0] for l in lines], [l[1] for l in lines])
        assert len(set(lab)) == CLUSTERS[name]
        # the tie rule matters: equal fractions taken the other way round give another forest
        other_ties = fm.kruskal(n, sorted(lines, key=lambda e: (-fm.fraction(e[2], e[3]), -e[0], -e[1])))
        assert sorted(other_ties) != sorted(f), name
        # the weights matter: the first spanning forest in line order is another one
        assert sorted(fm.kruskal(n, lines)) != sorted(f), name
        # fractions that occur on more than one forest edge
        fr = [fm.fraction(e[2], e[3]) for e in f]
        assert 4 <= sum(1 for v in set(fr) if fr.count(v) > 1) <= 10, name
        assert fm.forest_stdout_of_triangle(text, names).splitlines() == [e[4] for e in f]
    # the d3 forest cut at the smallest fraction of d1 (d2) is the d1 (d2) forest, and gives their recorded partitions
    for small in ("d1", "d2"):
        last = forests[small][-1]
        pre = fm.cut(forests["d3"], last[2], last[3])
        assert pre == forests[small] == forests["d3"][:len(pre)], small
        lines = fm.lines_of_stdout(texts[small], names)
        assert cm.labels(n, [e[0] for e in pre], [e[1] for e in pre]) == cm.labels(n, [l[0] for l in lines], [l[1] for l in lines])


def test_cut_property_on_random_graphs():
    rng = random.Random(5)
    for _ in range(30):
        n = rng.randint(2, 80)
        e = random_graph(rng, n, 4 * n, [8, 12, 24], 1)
        f = fm.forest(n, e)
        for numer, denom in ((1, 8), (1, 3), (1, 2), (5, 8), (11, 12), (1, 1)):
            thr = Fraction(numer, denom)
            sub = [x for x in e if fm.fraction(x[2], x[3]) >= thr]
            pre = fm.cut(f, numer, denom)
            assert pre == f[:len(pre)] == fm.forest(n, sub)
            assert cm.labels(n, [x[0] for x in pre], [x[1] for x in pre]) == cm.labels(n, [x[0] for x in sub], [x[1] for x in sub])


def test_key_lemma_exhaustively_up_to_128():
    fr = [(a, b) for b in range(1, 129) for a in range(0, b + 1)]
    keys = np.array([fm.key(a, b) for a, b in fr], dtype=np.uint64)
    vals = [Fraction(a, b) for a, b in fr]
    order = sorted(range(len(fr)), key=lambda i: vals[i])
    for i, j in zip(order, order[1:]):                                 # neighbours in fraction order decide every pair
        assert (keys[i] == keys[j]) == (vals[i] == vals[j]) and keys[i] <= keys[j], (fr[i], fr[j])
    assert fm.key(0, 0) == 0 and fm.key(5, 5) == 1 << 42


def test_key_lemma_on_random_pairs_up_to_the_limit():
    rng = random.Random(20261019)
    top = fm.DENOM_LIMIT - 1
    for t in range(200000):
        b, d = rng.randint(1, top), rng.randint(1, top)
        if t % 3 == 0:
            b, d = top - rng.randint(0, 3), top - rng.randint(0, 3)    # the closest fractions there are
        a = rng.randint(0, b)
        c = min(d, max(0, a * d // b + rng.randint(-1, 1)))            # a neighbour of a/b under d
        ka, kc = fm.key(a, b), fm.key(c, d)
        assert ka < 1 << 64 and kc < 1 << 64
        l, r = a * d, c * b
        assert (ka > kc) == (l > r) and (ka == kc) == (l == r), (a, b, c, d)


KEY_CHECK = r"""
#include <cstdio>
#include <cstdlib>
#include "forest_key.h"
int main()
{
    unsigned long long x = 20261019ull, bad = 0;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    const unsigned top = mg::FOREST_DENOM_LIMIT - 1;
    for (int t = 0; t < 2000000; t++) {
        unsigned b = 1 + (unsigned)(rnd() % top), d = t % 2 ? top - (unsigned)(rnd() % 4) : 1 + (unsigned)(rnd() % top);
        if (t % 4 == 3) b = top - (unsigned)(rnd() % 4);
        const unsigned a = (unsigned)(rnd() % (b + 1ull));
        long long c = (long long)((unsigned long long)a * d / b) + (long long)(rnd() % 3) - 1;
        if (c < 0) c = 0;
        if (c > d) c = d;
        const unsigned __int128 l = (unsigned __int128)a * d, r = (unsigned __int128)c * b;
        const unsigned long long ka = mg::forest_key(a, b), kc = mg::forest_key((unsigned)c, d);
        bad += (ka > kc) != (l > r) || (ka == kc) != (l == r);
        bad += mg::forest_before(a, b, 7, (unsigned)c, d, 9) != (l > r || l == r);
        bad += mg::forest_before(a, b, 9, (unsigned)c, d, 7) != (l > r);
    }
    bad += mg::forest_key(0, 0) != 0 || mg::forest_key(3, 3) != 1ull << 42 || mg::forest_rc(5, 2) != (5ull << 32 | 2);
    printf("%llu disagreements\n", bad);
    return bad != 0;
}
"""


def test_key_header_stands_alone_on_the_cpu(tmp_path):
    src = tmp_path / "key_check.cpp"
    src.write_text(KEY_CHECK)
    exe = str(tmp_path / "key_check")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "mash_amd", "csrc"), str(src), "-o", exe], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout == "0 disagreements\n", r.stdout + r.stderr[-2000:]
