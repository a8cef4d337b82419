"""The index build reads the table in place through the clustering's row map (host_index.cpp: order_rows, copy_rows; index_build.hip:
K0, K1, K3; compare_sparse.hip: the general sort's first kernel), makes the copy in clustered order only where copy suspects are
verified row against row, and asks whether the table holds copies of rows from a sample of every row (copy_gate.h).  n = 3 072 rows of s = 128 in 48 clusters of 64 rows, interleaved
row by row, so that the clustered order really permutes the rows; the inverted-index engine forced; every {numer, denom} of the
triangle against the oracle (compareSketches' merge loop) on every route:
the default (in place), the forced copy (same bytes), MASHGPU_SPARSE_INDEX=verify and =sort (the general sort through the map), a
refusal by the bucket sorts' order check (the general sort behind the tiles, through the map), a table with 40 true copies (the copy made for the
value-by-value check), a row that differs from another only where the gate does not look (a false suspect: no copy, the pair
as the oracle has it), and the default again with the fill running beside the build."""
import os
import re

import numpy as np
import pytest

from mash_amd import abi

from workloads import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, S, CLUSTERS = 3072, 128, 48
IN_PLACE, COPIED = "in clustered order, read in place", "in clustered order, copied"


@pytest.fixture(scope="module")
def eng():
    import torch                                           # (torch's HIP runtime initialises first: see test_gpu_parity.py)
    torch.cuda.init()
    e = abi.MashGpu(0)
    e.set_option("MASHGPU_COSTS_FIXED", "1")
    yield e
    e.close()


def _with_oracle(oracle, table, nhash, lengths):
    numer, denom, _, _ = oracle.triangle(table, nhash, lengths, 0, len(nhash), 21, 4.0 ** 21)
    return {"table": table, "nhash": nhash, "lengths": lengths, "numer": numer, "denom": denom}


def _with_rows_changed(oracle, base, table, nhash, rows):
    """the oracle's triangle of a table that differs from the base table in `rows` only: the pairs of those rows computed anew
    (the changed rows moved to the end of a reordered table, whose last rows the oracle is asked for; a pair's counts do not
    depend on which of the two rows comes first), every other pair taken from the base table's triangle, which stays as it is"""
    rows = np.asarray(sorted(rows))
    m, n = len(rows), len(nhash)
    perm = np.concatenate([np.setdiff1d(np.arange(n), rows), rows])
    nn, dd, _, _ = oracle.triangle(table[perm], nhash[perm], base["lengths"][perm], n - m, n, 21, 4.0 ** 21)
    numer, denom = base["numer"].copy(), base["denom"].copy()
    first = (n - m) * (n - m - 1) // 2
    for i in range(n - m, n):
        lo = i * (i - 1) // 2 - first
        hi_row, lo_row = np.maximum(perm[i], perm[:i]), np.minimum(perm[i], perm[:i])
        at = hi_row * (hi_row - 1) // 2 + lo_row
        numer[at], denom[at] = nn[lo:lo + i], dd[lo:lo + i]
    return {"table": table, "nhash": nhash, "lengths": base["lengths"], "numer": numer, "denom": denom}


@pytest.fixture(scope="module")
def base(oracle):
    """the table of every route but the two about copies, and its triangle by the oracle (computed once)"""
    table, nhash, lengths = synth.clustered_sketches(N, S, clusters=CLUSTERS, seed=61, pool=190, private=50)
    nhash = nhash.copy()
    nhash[777] = 0                                          # an empty row and a short one
    nhash[1500] = 40
    table[777, :] = np.uint64(abi.HASH_PAD)
    table[1500, 40:] = np.uint64(abi.HASH_PAD)
    return _with_oracle(oracle, table, nhash, lengths)


def _run(eng, case, monkeypatch, capfd, **env):
    """the whole triangle of a fresh table through the inverted-index engine; returns (records, what the build said)"""
    monkeypatch.setenv("MASHGPU_COMPARE_KERNEL", "sparse")
    monkeypatch.setenv("MASHGPU_SPARSE_DBG", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    t = eng.table_upload(case["table"], case["nhash"], case["lengths"])
    capfd.readouterr()
    try:
        got = eng.compare_tri_host(t)
    finally:
        t.free()
    err = capfd.readouterr().err
    assert "compare sparse: index of %d rows" % len(case["nhash"]) in err, err[-2000:]      # the engine asked for is the one that ran
    return got, err


def _check(got, case):
    assert np.array_equal(got["numer"], case["numer"]) and np.array_equal(got["denom"], case["denom"])


@pytest.fixture(scope="module")
def default_bytes():
    return {}


def test_default_reads_the_table_in_place(eng, base, default_bytes, monkeypatch, capfd):
    got, err = _run(eng, base, monkeypatch, capfd)
    assert IN_PLACE in err and "the copy gate had 0 suspects" in err and "index by tiles" in err, err[-2000:]
    _check(got, base)
    default_bytes["tri"] = got.tobytes()


def test_forced_copy_gives_the_same_bytes(eng, base, default_bytes, monkeypatch, capfd):
    if "tri" not in default_bytes:
        default_bytes["tri"] = _run(eng, base, monkeypatch, capfd)[0].tobytes()
    got, err = _run(eng, base, monkeypatch, capfd, MASHGPU_COMPARE_ROWCOPY="1")
    assert COPIED in err, err[-2000:]
    assert got.tobytes() == default_bytes["tri"]
    _check(got, base)


@pytest.mark.parametrize("mode", ["verify", "sort"])
def test_verify_and_sort_read_through_the_map(eng, base, mode, monkeypatch, capfd):
    got, err = _run(eng, base, monkeypatch, capfd, MASHGPU_SPARSE_INDEX=mode)      # (verify raises if an array of the two builds differs)
    assert IN_PLACE in err and ("index by tiles" in err) == (mode == "verify"), err[-2000:]
    _check(got, base)


def test_a_late_refusal_is_sorted_through_the_map(eng, base, monkeypatch, capfd):
    got, err = _run(eng, base, monkeypatch, capfd, MASHGPU_IX_DEBUG_SWAP="1")
    assert "clumped values: sorted instead" in err and IN_PLACE in err, err[-2000:]
    _check(got, base)


def test_true_copies_are_found_through_the_gate(eng, oracle, base, monkeypatch, capfd):
    table, nhash = base["table"].copy(), base["nhash"].copy()
    src = np.arange(40) * 70 + 11                           # 40 rows copied to 40 other places, some into other clusters
    dst = (src + 1000) % N
    table[dst], nhash[dst] = table[src], nhash[src]
    case = _with_rows_changed(oracle, base, table, nhash, dst)
    got, err = _run(eng, case, monkeypatch, capfd)
    assert "(40 copies of earlier rows)" in err and COPIED in err, err[-2000:]
    _check(got, case)


def _gate_positions(cnt):
    """copy_gate.h's rule, restated; checked against the header's own static_asserts"""
    src = open(os.path.join(ROOT, "mash_amd", "csrc", "copy_gate.h")).read()
    samples = int(re.search(r"COPY_GATE_SAMPLES = (\d+);", src).group(1))

    def position(k, c):
        return k if c <= samples else (k + 1) * c // samples - 1
    stated = re.findall(r"copy_gate_position\((\d+), (\d+)\) == (\d+)", src)
    assert len(stated) >= 6
    for k, c, p in stated:
        assert position(int(k), int(c)) == int(p), (k, c, p)
    return [position(k, cnt) for k in range(min(cnt, samples))]


def test_rows_that_differ_between_the_samples_are_no_copies(eng, oracle, base, monkeypatch, capfd):
    table, nhash = base["table"].copy(), base["nhash"].copy()
    a, b = 100, 100 + 5 * CLUSTERS                          # two rows of one cluster
    assert nhash[a] == S
    sampled = _gate_positions(S)
    assert sampled[-1] == S - 1 and len(sampled) == 32
    p = next(q for q in range(S // 2, S - 1) if q not in sampled)
    row = table[a].copy()
    v = int(row[p]) + 1                                     # between its neighbours: every other position stays
    if v >= int(row[p + 1]):
        v = int(row[p]) - 1
    assert int(row[p - 1]) < v < int(row[p + 1]) and v != int(row[p])
    row[p] = np.uint64(v)
    table[b], nhash[b] = row, nhash[a]
    case = _with_rows_changed(oracle, base, table, nhash, [b])
    got, err = _run(eng, case, monkeypatch, capfd)
    m = re.search(r"the copy gate had (\d+) suspects", err)
    assert m and int(m.group(1)) >= 1 and "(0 copies of earlier rows)" in err, err[-2000:]      # suspected, looked at in full, no copy
    _check(got, case)
    at = b * (b - 1) // 2 + a
    assert (int(got["numer"][at]), int(got["denom"][at])) == (int(case["numer"][at]), int(case["denom"][at]))
    assert int(case["numer"][at]) < S                       # (the oracle's pair is not that of two equal rows)


def test_default_beside_the_fill(eng, base, monkeypatch, capfd):
    eng.prof_enable(True)
    eng.prof_reset()
    try:
        got, err = _run(eng, base, monkeypatch, capfd, MASHGPU_FILL_ASIDE_MIN_PAIRS="1")
        aside = eng.prof_avg_ms("compare_fill_aside")[1]
    finally:
        eng.prof_enable(False)
    assert aside >= 1 and IN_PLACE in err, err[-2000:]
    _check(got, base)
