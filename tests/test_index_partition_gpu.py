"""K3 of the index build (index_build.hip: the tile partition) with both of its bodies -- the ranks taken in registers
(MASHGPU_IX_PARTITION=rank, the default) and the LSD sort in LDS (=lsd) -- the inverted-index engine forced.  The two tables of
test_index_offsets_counts_gpu.py, rebuilt here (n = 1 100 rows of s = 96: two full blocks of rows and a ragged third; full, short
and empty rows; one value held by 300 rows -- and n = 2 000 rows of s = 1 000, clusters interleaved row by row), and one of 600 rows
with s = 4 000 in which ten rows are full and the others hold a few dozen values: the plan then has few windows, and a full row
holds hundreds of entries in each -- across the 64 entries of a step, a wave's share and the tile's pieces.  With either body
MASHGPU_SPARSE_INDEX=verify finds no word that differs from the general sort's index, and every {numer, denom} of the triangle --
whole, and of a range of rows -- equals the oracle's (compareSketches' merge loop)."""
import re

import numpy as np
import pytest

from mash_amd import abi

from workloads import synth

pytestmark = pytest.mark.gpu

BODIES = ["rank", "lsd"]
NAMES = {"rank": "tile partition by ranks in registers (rank)", "lsd": "tile partition by the LSD sort in LDS (lsd)"}
TABLES = ["small", "large", "long_rows"]


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


@pytest.fixture(scope="module")
def small(oracle):
    """n = 1 100, s = 96 in 10 interleaved clusters; every eleventh row empty, every seventh short, one value in 300 rows"""
    n, s = 1100, 96
    table, nhash, lengths = synth.clustered_sketches(n, s, clusters=10, seed=17, pool=140, private=40)
    nhash = nhash.copy()
    rng = np.random.default_rng(3)
    common = np.uint64((1 << 52) + 12345)
    for r in range(n):
        c = int(nhash[r])
        if r % 11 == 5:
            c = 0
        elif r % 7 == 3:
            c = 1 + int(rng.integers(c - 1))
        h = table[r, :c].copy()
        if c and r < 900 and r % 3 == 0:
            h = np.unique(np.concatenate([h[:c - 1], [common]]))
        table[r, :] = np.uint64(abi.HASH_PAD)
        table[r, :len(h)] = h
        nhash[r] = len(h)
    assert int(((table == common).sum(axis=1) > 0).sum()) >= 250
    return _with_oracle(oracle, table, nhash, lengths)


@pytest.fixture(scope="module")
def large(oracle):
    """n = 2 000, s = 1 000 in 20 interleaved clusters (the benchmark's generator)"""
    from workloads import synth_torch
    h, nh, ln = synth_torch.clustered_sketch_table(2000, 1000, clusters=20, seed=23)
    return _with_oracle(oracle, h.cpu().numpy().view(np.uint64), nh.cpu().numpy().astype(np.uint32), ln.cpu().numpy().astype(np.uint64))


@pytest.fixture(scope="module")
def long_rows(oracle):
    """n = 600, s = 4 000: every sixtieth row holds 4 000 of a pool of 6 000 values, the others 5 to 40 of them -- 53 000 entries in
    a dozen windows or so, some 400 of a full row in each"""
    n, s = 600, 4000
    rng = np.random.default_rng(29)
    pool = np.unique(rng.integers(0, 1 << 62, size=6000, dtype=np.uint64))
    table = np.full((n, s), np.uint64(abi.HASH_PAD), dtype=np.uint64)
    nhash = np.zeros(n, dtype=np.uint32)
    for r in range(n):
        c = s if r % 60 == 7 else 5 + int(rng.integers(36))
        h = np.sort(rng.choice(pool, size=c, replace=False))
        table[r, :c] = h
        nhash[r] = c
    return _with_oracle(oracle, table, nhash, np.full(n, 1_000_000, dtype=np.uint64))


def _run(eng, case, monkeypatch, capfd, row_begin=0, row_end=None, **env):
    monkeypatch.setenv("MASHGPU_COMPARE_KERNEL", "sparse")
    monkeypatch.setenv("MASHGPU_SPARSE_DBG", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    t = eng.table_upload(case["table"], case["nhash"], case["lengths"])
    capfd.readouterr()
    try:
        got = eng.compare_tri_host(t, row_begin, row_end)
    finally:
        t.free()
    err = capfd.readouterr().err
    assert "compare sparse: index of %d rows" % len(case["nhash"]) in err, err[-2000:]      # the engine asked for is the one that ran
    return got, err


def _check(got, case, row_begin=0, row_end=None):
    row_end = len(case["nhash"]) if row_end is None else row_end
    a, b = row_begin * (row_begin - 1) // 2, row_end * (row_end - 1) // 2
    assert np.array_equal(got["numer"], case["numer"][a:b]) and np.array_equal(got["denom"], case["denom"][a:b])


@pytest.mark.parametrize("body", BODIES)
@pytest.mark.parametrize("which", TABLES)
def test_verify_finds_no_differing_word(eng, request, which, body, monkeypatch, capfd):
    case = request.getfixturevalue(which)
    got, err = _run(eng, case, monkeypatch, capfd, MASHGPU_SPARSE_INDEX="verify", MASHGPU_IX_PARTITION=body)      # (verify raises if an array differs)
    assert "index by tiles" in err and NAMES[body] in err and "sorted instead" not in err, err[-2000:]
    if which == "long_rows":                               # what the table is for: few windows, so hundreds of entries of a full row in each
        m = re.search(r"index by tiles: shift \d+, \d+ buckets \(\d+ per window, (\d+) windows\)", err)
        assert m and int(m.group(1)) <= 40, err[-2000:]
    _check(got, case)


@pytest.mark.parametrize("body", BODIES)
@pytest.mark.parametrize("which", TABLES)
def test_triangle_equals_the_oracle(eng, request, which, body, monkeypatch, capfd):
    case = request.getfixturevalue(which)
    got, err = _run(eng, case, monkeypatch, capfd, MASHGPU_IX_PARTITION=body)
    assert "index by tiles" in err and NAMES[body] in err and "sorted instead" not in err, err[-2000:]
    _check(got, case)


@pytest.mark.parametrize("body", BODIES)
@pytest.mark.parametrize("which", TABLES)
def test_row_range_equals_the_oracle(eng, request, which, body, monkeypatch, capfd):
    case = request.getfixturevalue(which)
    n = len(case["nhash"])
    b, e = n // 3 + 1, n - 7
    got, err = _run(eng, case, monkeypatch, capfd, row_begin=b, row_end=e, MASHGPU_IX_PARTITION=body)
    assert NAMES[body] in err, err[-2000:]
    _check(got, case, b, e)


def test_default_body_is_the_ranks(eng, large, monkeypatch, capfd):
    monkeypatch.delenv("MASHGPU_IX_PARTITION", raising=False)
    got, err = _run(eng, large, monkeypatch, capfd)
    assert "index by tiles" in err and NAMES["rank"] in err, err[-2000:]
    _check(got, large)
