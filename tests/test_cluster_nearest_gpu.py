"""`mash cluster -B` and mg_cluster_tri_nearest_host / mg_cluster_tri_nearest_dev on the device.

1. Through the command: for every recorded case of tests/golden/cluster (stdout of the REFERENCE CLI's `triangle -E`) the command
   prints, byte for byte, what tests/cluster_nearest_model.py makes of the recorded stdout -- on the candidate-list route, with the
   matrix route forced, with the matrix in row blocks of 100 pairs, with an edge list of 7 edges at first, with both, and on the host
   route (MASH_AMD_HOST_FINISH=1); stderr is the same on every route; the same with -C; and `mash cluster -R` without -B still
   prints what tests/cluster_greedy_model.py makes of the recording.
2. A band table whose answer has a closed form (rows i % 4 == 3 join the LATER representative, rows i % 4 == 2 are a tie).
3. Equal fractions under different denominators (32/64 beside 16/32) in both row orders, after the compared counts themselves
   have been checked to be that.
4. One species of 1 200 rows against the model over mg_compare_tri_results_host's records, in blocks and with short lists.
5. Calling conventions: the _dev form with a guard word, repeated calls, 0 and 1 rows, the error returns.
Here, and only here, workgroups race on best_key[] and rep[]: the emulator (tests/test_cluster_nearest_emu.py) runs them one after
another.  Every command runs under its own timeout; a non-zero exit ends the test.  The MG_ERR_UNSUPPORTED return for a sketch
size of 2^21 or more is not exercised (it would need a table of that width); it is one comparison in cluster_jobs (host_cluster.cpp)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from mash_amd import abi
from tests import cluster_greedy_model as gm
from tests import cluster_nearest_model as nm
from workloads import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASH = os.path.join(ROOT, "mash_amd", "bin", "mash")
GOLD = os.path.join(ROOT, "tests", "golden", "cluster")
KSPACE21 = 4.0 ** 21
MG_ERR_INVALID = -1             # include/mashgpu.h
PAD = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope="module")
def eng():
    import torch
    torch.cuda.init()          # (torch ships its own HIP runtime: it initialises first, tests/test_gpu_parity.py)
    e = abi.MashGpu(0)
    e.set_option("MASHGPU_COSTS_FIXED", "1")
    yield e
    e.close()


# ------------------------------------------------------------------------------------------ 1. through the command

CLI_ROUTES = {"lists": {}, "matrix": {"MASHGPU_RESULTS_MATRIX": "1"},
              "matrix in blocks of 100 pairs": {"MASHGPU_RESULTS_MATRIX": "1", "MASHGPU_CLUSTER_BLOCK_PAIRS": "100"},
              "a list of 7 edges at first": {"MASHGPU_GREEDY_EDGE_CAP": "7"},
              "blocks and a short list": {"MASHGPU_RESULTS_MATRIX": "1", "MASHGPU_CLUSTER_BLOCK_PAIRS": "100", "MASHGPU_GREEDY_EDGE_CAP": "7"},
              "host": {"MASH_AMD_HOST_FINISH": "1"}}


def mash(args, cwd, extra_env):
    env = dict(os.environ)
    for k in ("MASH_AMD_HOST_FINISH", "MASHGPU_RESULTS_MATRIX", "MASHGPU_CLUSTER_BLOCK_PAIRS", "MASHGPU_GREEDY_EDGE_CAP"):
        env.pop(k, None)
    env.update(extra_env)
    r = subprocess.run([MASH, *args], cwd=cwd, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def cluster_options(triangle_options):
    """triangle's -d defaults to 1, cluster's to 0.05: a recording without -d is matched by an explicit -d 1"""
    return list(triangle_options) if "-d" in triangle_options else ["-d", "1", *triangle_options]


def recorded():
    cases = json.load(open(os.path.join(GOLD, "cases.json")))
    return cases, {c["name"]: open(os.path.join(GOLD, c["name"] + ".out")).read() for c in cases["cases"]}


@pytest.mark.parametrize("name", ["d1", "d2", "d3", "v", "dv"])
def test_command_on_the_recorded_family_every_route(name):
    cases, texts = recorded()
    c = [x for x in cases["cases"] if x["name"] == name][0]
    want = nm.nearest_stdout_of_triangle(texts[name], cases["names"])
    first = gm.greedy_stdout_of_triangle(texts[name], cases["names"])
    if name != "d3":                                                # (d3: the two rules agree, the fourth field apart)
        assert [ln.rsplit("\t", 1)[0] for ln in want.splitlines()] != first.splitlines()
    args = [*cases["sketch"], *cluster_options(c["options"]), cases["input"]]
    errs = set()
    for route, env in CLI_ROUTES.items():
        r = mash(["cluster", "-B", *args], GOLD, env)
        assert r.stdout == want, (name, route)
        errs.add(r.stderr)
    assert len(errs) == 1
    assert mash(["cluster", "-R", "-B", *args], GOLD, {}).stdout == want          # -B implies -R
    assert mash(["cluster", "-R", *args], GOLD, {}).stdout == first               # without -B nothing has changed


def test_command_with_comments():
    cases, texts = recorded()
    for name in ("d2", "dv"):
        opts = cluster_options([c["options"] for c in cases["cases"] if c["name"] == name][0])
        want_c = nm.nearest_stdout_of_triangle(texts[name], cases["names"], cases["comments"])
        for route in ("lists", "matrix in blocks of 100 pairs", "host"):
            r = mash(["cluster", "-B", "-C", *cases["sketch"], *opts, cases["input"]], GOLD, CLI_ROUTES[route])
            assert r.stdout == want_c, (name, route)


# ------------------------------------------------------------------------------------------ through the C ABI

def with_options(eng, opts, fn):
    for o, v in opts.items():
        eng.set_option(o, v)
    try:
        return fn()
    finally:
        for o in opts:
            eng.set_option(o, None)


def window_table(n, s, step, seed):
    """row i is the window pool[i * step : i * step + s] of one ascending pool of distinct hashes: the pair (i, i + k) shares
    s - k * step of the s smallest values of its union -- shared = s - k * step over denom = s"""
    rng = np.random.default_rng(seed)
    need = (n - 1) * step + s
    pool = np.unique(rng.integers(0, 1 << 54, need + need // 8 + 64, dtype=np.uint64))[:need]
    assert len(pool) == need
    idx = (np.arange(n, dtype=np.int64) * step)[:, None] + np.arange(s, dtype=np.int64)[None, :]
    return pool[idx], np.full(n, s, dtype=np.uint32), np.full(n, 1_000_000, dtype=np.uint64)


def mash_distance(shared, s, k=21):
    j = shared / s
    return -np.log(2 * j / (1 + j)) / k


def test_band_table_with_a_closed_form(eng):
    """2. window_table(300, 1000, 100), threshold between 3 and 4 steps: representatives are the rows i % 4 == 0; row 4g + 3 shares 900
    with the later representative and 700 with the earlier one; row 4g + 2 shares 800 with both and stays with the smaller; row 299 has
    no later representative"""
    n, s, step = 300, 1000, 100
    table, nh, lengths = window_table(n, s, step, seed=5)
    t = eng.table_upload(table, nh, lengths)
    d = [mash_distance(s - k * step, s) for k in range(6)]
    band_d = (d[3] + d[4]) / 2
    i = np.arange(n)
    want = np.where((i % 4 == 3) & (i + 1 < n), i + 1, i - i % 4).astype(np.uint32)
    assert want[2] == 0 and want[3] == 4 and want[298] == 296 and want[299] == 296
    routes = {"default": {}, "matrix": {"MASHGPU_RESULTS_MATRIX": "1"},
              "blocks of 4097 pairs, a list of 1 edge": {"MASHGPU_RESULTS_MATRIX": "1", "MASHGPU_CLUSTER_BLOCK_PAIRS": "4097", "MASHGPU_GREEDY_EDGE_CAP": "1"}}
    for route, opts in routes.items():
        rep, nc, ne = with_options(eng, opts, lambda: eng.cluster_tri_nearest_host(t, 21, KSPACE21, band_d, -1.0))
        print(f"band route {route}: edges {ne} clusters {nc} {eng.cluster_greedy_stats()}")
        assert ne == 3 * n - 6, route
        assert np.array_equal(rep, want), (route, np.nonzero(rep != want)[0][:10])
        assert nc == n // 4, route
    first, nc1, ne1 = eng.cluster_tri_greedy_host(t, 21, KSPACE21, band_d, -1.0)
    assert np.array_equal(first, (i - i % 4).astype(np.uint32)) and (nc1, ne1) == (n // 4, 3 * n - 6)
    t.free()


def test_equal_fractions_under_different_denominators(eng):
    """3. s = 64.  A has 64 hashes that contain the member's 32: 32/64.  B has 16 hashes, all among the member's: the union is the
    member's 32 hashes, 16/32.  B's hashes are among A's: A and B share 16/64, beyond -d 0.03 (32/64 and 16/32 are within it).  In
    both row orders the member joins row 0."""
    s = 64
    pool = np.unique(np.random.default_rng(9).integers(0, 1 << 54, 200, dtype=np.uint64))[:64]
    a = pool                                                       # 64 hashes
    m = pool[::2]                                                  # 32 of them
    b = m[::2]                                                     # 16 of those
    rows = {"A": a, "M": m, "B": b}
    for order in (("A", "M", "B"), ("B", "M", "A")):
        table = np.full((3, s), PAD, dtype=np.uint64)
        nh = np.zeros(3, dtype=np.uint32)
        for r, name in enumerate(order):
            table[r, :len(rows[name])] = np.sort(rows[name])
            nh[r] = len(rows[name])
        t = eng.table_upload(table, nh, np.full(3, 1_000_000, dtype=np.uint64))
        rec = eng.compare_tri_results(t, 21, KSPACE21, 0.03, -1.0)
        got = {(int(x["row"]), int(x["col"])): (int(x["numer"]), int(x["denom"])) for x in rec}
        assert set(got) == {(1, 0), (2, 1)}, (order, got)           # the two representatives are apart
        (n0, d0), (n2, d2) = got[(1, 0)], got[(2, 1)]
        assert n0 * d2 == n2 * d0 and d0 != d2 and {(n0, d0), (n2, d2)} == {(32, 64), (16, 32)}, (order, got)
        every = eng.compare_tri_host(t)                            # the flat triangle: (1, 0), (2, 0), (2, 1)
        assert (int(every["numer"][1]), int(every["denom"][1])) == (16, 64), (order, every)
        for route, opts in {"default": {}, "matrix": {"MASHGPU_RESULTS_MATRIX": "1"}}.items():
            rep, nc, ne = with_options(eng, opts, lambda: eng.cluster_tri_nearest_host(t, 21, KSPACE21, 0.03, -1.0))
            assert list(rep) == [0, 0, 2] and (nc, ne) == (2, 2), (order, route, list(rep))
        t.free()


def test_one_species_blocks_and_list_sizes(eng):
    """4. rep, clusters and edges against the model over mg_compare_tri_results_host's records; the matrix route in row blocks of one
    pair, of 4097 and in one block; first capacities of 1 edge, 63, one short and exactly enough"""
    n = 1200
    table, nh, lengths = synth.species_sketches(n, 1000, seed=7)
    t = eng.table_upload(table, nh, lengths)
    for max_d in (0.05, 0.03):
        rec = eng.compare_tri_results(t, 21, KSPACE21, max_d, -1.0, capacity=1 << 22)
        ne_want = len(rec)
        want = np.array(nm.nearest_fast(n, rec["row"], rec["col"], rec["numer"], rec["denom"]), dtype=np.uint32)
        first, nc_first, ne_first = eng.cluster_tri_greedy_host(t, 21, KSPACE21, max_d, -1.0)
        assert ne_first == ne_want > 64
        routes = {f"blocks of {b} pairs": {"MASHGPU_RESULTS_MATRIX": "1", "MASHGPU_CLUSTER_BLOCK_PAIRS": str(b)} for b in (1, 4097, 1 << 30)}
        routes.update({f"a list of {c} edges at first": {"MASHGPU_GREEDY_EDGE_CAP": str(c)} for c in (1, 63, ne_want - 1, ne_want)})
        stats = {}
        for route, opts in routes.items():
            rep, nc, ne = with_options(eng, opts, lambda: eng.cluster_tri_nearest_host(t, 21, KSPACE21, max_d, -1.0))
            stats[route] = st = eng.cluster_greedy_stats()
            print(f"species d {max_d} route {route}: edges {ne} clusters {nc} {st}, {int((rep != first).sum())} members moved, {int((rep > np.arange(n)).sum())} to a later one")
            assert ne == ne_want, (max_d, route)
            assert np.array_equal(rep, want), (max_d, route, int((rep != want).sum()))
            assert nc == nc_first == int((want == np.arange(n)).sum()), (max_d, route)
            assert np.array_equal(np.nonzero(rep == np.arange(n))[0], np.nonzero(first == np.arange(n))[0]), (max_d, route)
            assert 1 <= st["rounds"] <= n and st["batches"] >= 1 and st["edge_capacity"] >= ne
        assert stats[f"a list of {ne_want} edges at first"]["regrows"] == 0 and stats[f"a list of {ne_want - 1} edges at first"]["regrows"] == 1
        assert stats["a list of 1 edges at first"]["regrows"] >= 1
        assert (want != first).any(), max_d                         # at least one member is not under its first representative
    t.free()


# ------------------------------------------------------------------------------------------ 5. calling conventions

def test_dev_form_and_repeated_calls(eng):
    import torch
    n = 1200
    table, nh, lengths = synth.species_sketches(n, 1000, seed=4)
    t = eng.table_upload(table, nh, lengths)
    first = eng.cluster_tri_nearest_host(t, 21, KSPACE21, 0.03, -1.0)
    for _ in range(2):
        d_rep = torch.full((n + 1,), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
        nc, ne = eng.cluster_tri_nearest_dev(t, 21, KSPACE21, d_rep.data_ptr(), 0.03, -1.0)
        torch.cuda.synchronize()
        got = d_rep.cpu().numpy().view(np.uint32)
        assert got[n] == 0x7FFFFFFF and np.array_equal(got[:n], first[0]) and (nc, ne) == first[1:]
    again = eng.cluster_tri_nearest_host(t, 21, KSPACE21, 0.03, -1.0)
    assert np.array_equal(again[0], first[0]) and again[1:] == first[1:]
    t.free()


def test_tables_of_no_and_one_row(eng):
    one = np.sort(np.random.default_rng(1).integers(0, 1 << 54, (1, 64), dtype=np.uint64), axis=1)
    t = eng.table_upload(one, np.full(1, 64, dtype=np.uint32), np.full(1, 1000, dtype=np.uint64))
    rep, nc, ne = eng.cluster_tri_nearest_host(t, 21, KSPACE21, 0.05, -1.0)
    assert list(rep) == [0] and (nc, ne) == (1, 0)
    t.free()
    t = eng.table_upload(np.zeros((0, 64), dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint64))
    rep, nc, ne = eng.cluster_tri_nearest_host(t, 21, KSPACE21, 0.05, -1.0)
    assert len(rep) == 0 and (nc, ne) == (0, 0)
    t.free()


def test_error_returns(eng):
    table, nh, lengths = synth.clustered_sketches(96, 1000, clusters=3, seed=1)
    t = eng.table_upload(table, nh, lengths)
    bare = eng.table_upload(table, nh, None)
    rep = np.zeros(96, dtype=np.uint32)
    nc, ne = C.c_uint64(0), C.c_uint64(0)

    def call(fn, max_d, max_p, k=21, table=t, out=rep.ctypes.data, nc_ref=C.byref(nc)):
        return fn(eng.ctx, table.handle if table is not None else None, k, KSPACE21, max_d, max_p, out, nc_ref, C.byref(ne))

    for fn in (eng.lib.mg_cluster_tri_nearest_host, eng.lib.mg_cluster_tri_nearest_dev):
        for max_d, max_p in ((-1.0, -1.0), (1.0, 1.0), (1.0, -1.0), (2.0, 1.5)):
            assert call(fn, max_d, max_p) == MG_ERR_INVALID
            assert b"both filters are off" in eng.lib.mg_last_error(eng.ctx)
        assert call(fn, 0.05, -1.0, out=None) == MG_ERR_INVALID and b"NULL argument" in eng.lib.mg_last_error(eng.ctx)
        assert call(fn, 0.05, -1.0, table=None) == MG_ERR_INVALID
        assert call(fn, 0.05, -1.0, nc_ref=None) == MG_ERR_INVALID
        assert call(fn, 0.05, -1.0, table=bare) == MG_ERR_INVALID and b"no lengths" in eng.lib.mg_last_error(eng.ctx)
    assert call(eng.lib.mg_cluster_tri_nearest_host, 0.05, -1.0, k=0) == MG_ERR_INVALID
    assert call(eng.lib.mg_cluster_tri_nearest_host, 0.05, -1.0) == abi.MG_OK and int(nc.value) == 3      # the context still works
    bare.free()
    t.free()
