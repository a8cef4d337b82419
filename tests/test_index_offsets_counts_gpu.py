"""The window offsets and the blocks' bucket counts from one read of the table (index_build.hip: ix_offsets_counts_kernel; the early
call of host_index.cpp: order_rows) against K0 + K1 (MASHGPU_IX_COUNTS=tiles), the inverted-index engine forced.  Two tables whose
clusters are interleaved row by row, so that the index is built through a row map that really permutes: n = 1 100 rows of s = 96
(two full blocks of rows and a ragged third; full, short and empty rows; one value held by 300 rows) and n = 2 000 rows of s = 1 000
(workloads/synth_torch).  On both routes MASHGPU_SPARSE_INDEX=verify finds no word that differs from the general sort's index, and
every {numer, denom} of the triangle -- whole, and of a range of rows -- equals the oracle's (compareSketches' merge loop)."""
import numpy as np
import pytest

from mash_amd import abi

from workloads import synth

pytestmark = pytest.mark.gpu

IN_PLACE = "in clustered order, read in place"
FUSED, TILES = "block counts made with the window offsets", "block counts by the tiles (K1)"
ROUTES = ["fused", "tiles"]


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


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("which", ["small", "large"])
def test_verify_finds_no_differing_word(eng, request, which, route, monkeypatch, capfd):
    case = request.getfixturevalue(which)
    got, err = _run(eng, case, monkeypatch, capfd, MASHGPU_SPARSE_INDEX="verify", MASHGPU_IX_COUNTS=route)      # (verify raises if an array differs)
    assert IN_PLACE in err and "index by tiles" in err and "sorted instead" not in err, err[-2000:]
    assert (FUSED if route == "fused" else TILES) in err, err[-2000:]
    _check(got, case)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("which", ["small", "large"])
def test_triangle_equals_the_oracle(eng, request, which, route, monkeypatch, capfd):
    case = request.getfixturevalue(which)
    got, err = _run(eng, case, monkeypatch, capfd, MASHGPU_IX_COUNTS=route)
    assert IN_PLACE in err and (FUSED if route == "fused" else TILES) in err, err[-2000:]
    _check(got, case)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("which", ["small", "large"])
def test_row_range_equals_the_oracle(eng, request, which, route, monkeypatch, capfd):
    case = request.getfixturevalue(which)
    n = len(case["nhash"])
    b, e = n // 3 + 1, n - 7
    got, _ = _run(eng, case, monkeypatch, capfd, row_begin=b, row_end=e, MASHGPU_IX_COUNTS=route)
    _check(got, case, b, e)


def test_default_route_is_the_fused_kernel(eng, large, monkeypatch, capfd):
    got, err = _run(eng, large, monkeypatch, capfd)
    assert IN_PLACE in err and FUSED in err, err[-2000:]
    _check(got, large)
