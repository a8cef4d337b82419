"""`mash cluster -R` and mg_cluster_tri_greedy_host / mg_cluster_tri_greedy_dev on the device.

Through the command: for every recorded case of tests/golden/cluster (stdout of the REFERENCE CLI's `triangle -E`) the command
prints, byte for byte, what tests/cluster_greedy_model.py makes of the recorded stdout -- on the candidate-list route, with the
matrix route forced, with the matrix in row blocks of a few pairs, with an edge list that starts too short, and on the host
route (MASH_AMD_HOST_FINISH=1); the same with -C.
Through the C ABI: rep, clusters and edges against the model over the records of mg_compare_tri_results_host (the existing,
oracle-verified call) on the same table and filters, on every route, in one block and in many, and with a
MASHGPU_GREEDY_EDGE_CAP small enough to force the regrow: a C3-style table of 20 000 rows, one species of 4 096, a synthetic
table whose threshold graph is a path or a band in index order (5 000 rows: thousands of rounds), tables of 0 and 1 rows.
Here, and only here, workgroups race on the state array: the emulator (tests/test_cluster_greedy_emu.py) runs them one after
another.  Every command runs under its own timeout.
NOT RUN YET: when this file was written no device run could be obtained; it has been collected, not executed."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from mash_amd import abi
from tests import cluster_greedy_model as gm
from tests import cluster_model as cm
from workloads import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASH = os.path.join(ROOT, "mash_amd", "bin", "mash")
GOLD = os.path.join(ROOT, "tests", "golden", "cluster")
KSPACE21 = 4.0 ** 21
MG_ERR_INVALID = -1             # include/mashgpu.h

# the two routes of the thresholded compare (candidate lists; row blocks of the matrix), the matrix in many blocks, and an edge
# list that starts with room for 1 000 edges and has to be regrown
ROUTES = {"default": {}, "matrix": {"MASHGPU_RESULTS_MATRIX": "1"},
          "blocks": {"MASHGPU_RESULTS_MATRIX": "1", "MASHGPU_CLUSTER_BLOCK_PAIRS": "2000000"},
          "short list": {"MASHGPU_GREEDY_EDGE_CAP": "1000"},
          "blocks, short list": {"MASHGPU_RESULTS_MATRIX": "1", "MASHGPU_CLUSTER_BLOCK_PAIRS": "2000000", "MASHGPU_GREEDY_EDGE_CAP": "1000"}}


@pytest.fixture(scope="module")
def eng():
    import torch
    torch.cuda.init()          # (torch ships its own HIP runtime: it initialises first, tests/test_gpu_parity.py)
    e = abi.MashGpu(0)
    e.set_option("MASHGPU_COSTS_FIXED", "1")
    yield e
    e.close()


# ------------------------------------------------------------------------------------------ through the command

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


def test_command_on_the_recorded_family_every_route():
    cases, texts = recorded()
    seen = set()
    for c in cases["cases"]:
        want = gm.greedy_stdout_of_triangle(texts[c["name"]], cases["names"])
        assert want != cm.cluster_stdout_of_triangle(texts[c["name"]], cases["names"])      # not what `mash cluster` prints without -R
        seen.add(want)
        args = ["cluster", "-R", *cases["sketch"], *cluster_options(c["options"]), cases["input"]]
        errs = set()
        for route, env in CLI_ROUTES.items():
            r = mash(args, GOLD, env)
            assert r.stdout == want, (c["name"], route)
            errs.add(r.stderr)
        assert len(errs) == 1
    assert len(seen) == 5                                          # five cases, five partitions


def test_command_with_comments_and_without_r():
    cases, texts = recorded()
    for name in ("d2", "dv"):
        opts = cluster_options([c["options"] for c in cases["cases"] if c["name"] == name][0])
        want_c = gm.greedy_stdout_of_triangle(texts[name], cases["names"], cases["comments"])
        for route in ("lists", "matrix in blocks of 100 pairs", "host"):
            r = mash(["cluster", "-R", "-C", *cases["sketch"], *opts, cases["input"]], GOLD, CLI_ROUTES[route])
            assert r.stdout == want_c, (name, route)
        # without -R nothing has changed
        r = mash(["cluster", *cases["sketch"], *opts, cases["input"]], GOLD, {})
        assert r.stdout == cm.cluster_stdout_of_triangle(texts[name], cases["names"])


def test_command_default_distance_is_0_05():
    cases, texts = recorded()
    want = gm.greedy_stdout_of_triangle(texts["d3"], cases["names"])
    for env in ({}, {"MASH_AMD_HOST_FINISH": "1"}):
        assert mash(["cluster", "-R", *cases["sketch"], cases["input"]], GOLD, env).stdout == want


# ------------------------------------------------------------------------------------------ through the C ABI

def with_options(eng, opts, fn):
    for o, v in opts.items():
        eng.set_option(o, v)
    try:
        return fn()
    finally:
        for o in opts:
            eng.set_option(o, None)


def check_table(eng, t, n, filters, routes=ROUTES, k=21, kspace=KSPACE21, capacity=1 << 22):
    """rep, clusters and edges of every filter on every route against the model over mg_compare_tri_results_host's records;
    -> {filter: (rep, edges, {route: stats})}"""
    out = {}
    for fname, (max_d, max_p) in filters.items():
        rec = eng.compare_tri_results(t, k, kspace, max_d, max_p, capacity=capacity)
        want = np.array(gm.reps_fast(n, rec["row"], rec["col"]), dtype=np.uint32)
        _, _, ne_single = eng.cluster_tri_host(t, k, kspace, max_d, max_p)
        assert ne_single == len(rec)
        stats = {}
        for route, opts in routes.items():
            rep, nc, ne = with_options(eng, opts, lambda: eng.cluster_tri_greedy_host(t, k, kspace, max_d, max_p))
            st = eng.cluster_greedy_stats()
            print(f"n {n} filter {fname} route {route}: edges {ne} clusters {nc} {st}")
            assert ne == len(rec) == ne_single, (fname, route, ne, len(rec))
            assert np.array_equal(rep, want), (fname, route, int((rep != want).sum()))
            assert nc == int((want == np.arange(n)).sum()), (fname, route)
            assert 1 <= st["rounds"] <= n and st["batches"] >= 1 and st["edge_capacity"] >= ne
            if "MASHGPU_GREEDY_EDGE_CAP" in opts and ne > int(opts["MASHGPU_GREEDY_EDGE_CAP"]):
                assert st["regrows"] >= 1, (fname, route, st)
            stats[route] = st
        out[fname] = (want, len(rec), stats)
    return out


def test_c3_style_table_every_route(eng):
    n = 20000
    table, nh, lengths = synth.clustered_sketches(n, 1000, clusters=n // 100, seed=3)
    t = eng.table_upload(table, nh, lengths)
    res = check_table(eng, t, n, {"d": (0.05, -1.0), "both": (0.05, 1e-10)})
    rep, ne, stats = res["d"]
    assert 0 < ne < n * (n - 1) // 2 and 1 < len(set(rep.tolist())) < n     # the filter bites, and something is joined
    assert stats["short list"]["regrows"] >= 1 and stats["default"]["regrows"] == 0
    t.free()


def test_one_species_is_not_what_single_linkage_gives(eng):
    n = 4096
    table, nh, lengths = synth.species_sketches(n, 1000, seed=1)
    t = eng.table_upload(table, nh, lengths)
    res = check_table(eng, t, n, {"d": (0.05, -1.0), "d.03": (0.03, -1.0), "v": (-1.0, 1e-10)})
    for fname in ("d", "d.03"):
        rep, ne, _ = res[fname]
        lab, _, _ = eng.cluster_tri_host(t, 21, KSPACE21, *{"d": (0.05, -1.0), "d.03": (0.03, -1.0)}[fname])
        assert ne > 0 and not np.array_equal(rep, lab)             # chains: the greedy partition is finer
        assert np.array_equal(lab[rep], lab)                       # ... and refines the single-linkage one
    t.free()


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


def test_path_and_band_in_index_order_take_thousands_of_rounds(eng):
    n, s, step = 5000, 1000, 100
    table, nh, lengths = window_table(n, s, step, seed=5)
    t = eng.table_upload(table, nh, lengths)
    d = [mash_distance(s - k * step, s) for k in range(6)]
    path_d, band_d = (d[1] + d[2]) / 2, (d[3] + d[4]) / 2           # edges (i, i + 1) alone; edges (i, i + k), k <= 3
    routes = {r: ROUTES[r] for r in ("default", "matrix", "blocks, short list")}
    res = check_table(eng, t, n, {"path": (path_d, -1.0), "band": (band_d, -1.0)}, routes=routes)
    rep, ne, stats = res["path"]
    assert ne == n - 1 and np.array_equal(rep, np.arange(n, dtype=np.uint32) & ~np.uint32(1))      # every other row
    # row i cannot be decided before row i - 1, and a round decides two rows of a path at most (a representative in its part B,
    # the next row in the part A behind it, whose successor may already be free in the same round): n / 2 rounds at least
    for route, st in stats.items():
        assert n // 2 <= st["rounds"] <= n and st["batches"] >= 10, (route, st)
    rep, ne, stats = res["band"]
    assert ne == 3 * n - 6 and np.array_equal(rep, (np.arange(n) // 4 * 4).astype(np.uint32))
    for route, st in stats.items():
        assert n // 4 <= st["rounds"] <= n, (route, st)
    t.free()


def test_block_boundaries_and_list_sizes(eng):
    """the matrix route in row blocks of one row, of a few rows and in one block; first capacities of 1 edge, of a few and of
    exactly the number of edges"""
    n = 1200
    table, nh, lengths = synth.species_sketches(n, 1000, seed=7)
    t = eng.table_upload(table, nh, lengths)
    ne = len(eng.compare_tri_results(t, 21, KSPACE21, 0.05, -1.0, capacity=1 << 22))
    routes = {f"blocks of {b} pairs": {"MASHGPU_RESULTS_MATRIX": "1", "MASHGPU_CLUSTER_BLOCK_PAIRS": str(b)} for b in (1, 4097, 1 << 30)}
    routes.update({f"a list of {c} edges at first": {"MASHGPU_GREEDY_EDGE_CAP": str(c)} for c in (1, 63, ne - 1, ne)})
    routes["blocks of 4097 pairs, a list of 1 edge"] = {"MASHGPU_RESULTS_MATRIX": "1", "MASHGPU_CLUSTER_BLOCK_PAIRS": "4097", "MASHGPU_GREEDY_EDGE_CAP": "1"}
    res = check_table(eng, t, n, {"d": (0.05, -1.0)}, routes=routes)
    stats = res["d"][2]
    assert ne > 64 and stats[f"a list of {ne} edges at first"]["regrows"] == 0 and stats[f"a list of {ne - 1} edges at first"]["regrows"] == 1
    t.free()


# ------------------------------------------------------------------------------------------ calling conventions

def test_dev_form_and_repeated_calls(eng):
    import torch
    n = 4096
    table, nh, lengths = synth.species_sketches(n, 1000, seed=4)
    t = eng.table_upload(table, nh, lengths)
    for route, opts in ROUTES.items():
        first = with_options(eng, opts, lambda: eng.cluster_tri_greedy_host(t, 21, KSPACE21, 0.03, -1.0))
        again = with_options(eng, opts, lambda: eng.cluster_tri_greedy_host(t, 21, KSPACE21, 0.03, -1.0))
        assert np.array_equal(again[0], first[0]) and again[1:] == first[1:], route
        d_rep = torch.full((n + 1,), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
        nc, ne = with_options(eng, opts, lambda: eng.cluster_tri_greedy_dev(t, 21, KSPACE21, d_rep.data_ptr(), 0.03, -1.0))
        torch.cuda.synchronize()
        got = d_rep.cpu().numpy().view(np.uint32)
        assert got[n] == 0x7FFFFFFF and np.array_equal(got[:n], first[0]) and (nc, ne) == first[1:], route
    t.free()


def test_tables_of_no_and_one_row(eng):
    one = np.sort(np.random.default_rng(1).integers(0, 1 << 54, (1, 64), dtype=np.uint64), axis=1)
    t = eng.table_upload(one, np.full(1, 64, dtype=np.uint32), np.full(1, 1000, dtype=np.uint64))
    rep, nc, ne = eng.cluster_tri_greedy_host(t, 21, KSPACE21, 0.05, -1.0)
    assert list(rep) == [0] and (nc, ne) == (1, 0)
    t.free()
    t = eng.table_upload(np.zeros((0, 64), dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint64))
    rep, nc, ne = eng.cluster_tri_greedy_host(t, 21, KSPACE21, 0.05, -1.0)
    assert len(rep) == 0 and (nc, ne) == (0, 0)
    t.free()


def test_error_returns(eng):
    table, nh, lengths = synth.clustered_sketches(96, 1000, clusters=3, seed=1)
    t = eng.table_upload(table, nh, lengths)
    rep = np.zeros(96, dtype=np.uint32)
    nc, ne = C.c_uint64(0), C.c_uint64(0)

    def call(fn, max_d, max_p, k=21, table=t, out=rep.ctypes.data):
        return fn(eng.ctx, table.handle, k, KSPACE21, max_d, max_p, out, C.byref(nc), C.byref(ne))

    for fn in (eng.lib.mg_cluster_tri_greedy_host, eng.lib.mg_cluster_tri_greedy_dev):
        for max_d, max_p in ((-1.0, -1.0), (1.0, 1.0), (1.0, -1.0), (2.0, 1.5)):
            assert call(fn, max_d, max_p) == MG_ERR_INVALID
            assert b"both filters are off" in eng.lib.mg_last_error(eng.ctx)
        assert call(fn, 0.05, -1.0, out=None) == MG_ERR_INVALID
    assert call(eng.lib.mg_cluster_tri_greedy_host, 0.05, -1.0, k=0) == MG_ERR_INVALID
    assert call(eng.lib.mg_cluster_tri_greedy_host, 0.05, -1.0) == abi.MG_OK and int(nc.value) == 3      # the context still works
    t.free()
