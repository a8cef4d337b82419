"""`mash cluster -T` and mg_cluster_tri_forest_host on the device.

Through the command: for every recorded case of tests/golden/cluster (stdout of the REFERENCE CLI's `triangle -E`) the command
prints, byte for byte, what tests/forest_model.py makes of the recorded stdout -- on the candidate-list route, with the matrix route
forced, with the matrix in row blocks of 100 pairs, with an edge list of 7 edges at first, with both, and on the host route
(MASH_AMD_HOST_FINISH=1); the same with -C; `mash cluster` and `mash cluster -R` print what they printed before.
Through the C ABI: the records field by field (the doubles bitwise), label, clusters and edges against the model over the records of
mg_compare_tri_results_host (the existing, oracle-verified call) and against mg_cluster_tri_host on the same table and filters, on
every route, in one block and in many, and with a MASHGPU_FOREST_EDGE_CAP small enough to force the regrow: a C3-style table of
20 000 rows, one species of 4 096 (millions of edges, long runs of equal fractions), a synthetic table whose threshold graph is a
path or a band in index order (5 000 rows: at most 13 rounds where the greedy rounds need thousands), a ragged table whose passing
edges carry many denominators, tables of 0 and 1 rows.
Here, and only here, workgroups race on best_key / best_rc and on the union-find: the emulator (tests/test_forest_emu.py) runs them
one after another.  Every command runs under its own timeout."""
import ctypes as C
import json
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from mash_amd import abi
from tests import cluster_greedy_model as gm
from tests import cluster_model as cm
from tests import forest_model as fm
from workloads import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASH = os.path.join(ROOT, "mash_amd", "bin", "mash")
GOLD = os.path.join(ROOT, "tests", "golden", "cluster")
KSPACE21 = 4.0 ** 21
MG_ERR_INVALID, MG_ERR_NOMEM = -1, -4          # include/mashgpu.h
PAD = np.uint64(0xFFFFFFFFFFFFFFFF)

# the two routes of the thresholded compare (candidate lists; row blocks of the matrix), the matrix in many blocks, and an edge
# list that starts with room for 1 000 edges and has to be regrown
ROUTES = {"default": {}, "matrix": {"MASHGPU_RESULTS_MATRIX": "1"},
          "blocks": {"MASHGPU_RESULTS_MATRIX": "1", "MASHGPU_CLUSTER_BLOCK_PAIRS": "2000000"},
          "short list": {"MASHGPU_FOREST_EDGE_CAP": "1000"},
          "blocks, short list": {"MASHGPU_RESULTS_MATRIX": "1", "MASHGPU_CLUSTER_BLOCK_PAIRS": "2000000", "MASHGPU_FOREST_EDGE_CAP": "1000"}}


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
              "a list of 7 edges at first": {"MASHGPU_FOREST_EDGE_CAP": "7"},
              "blocks and a short list": {"MASHGPU_RESULTS_MATRIX": "1", "MASHGPU_CLUSTER_BLOCK_PAIRS": "100", "MASHGPU_FOREST_EDGE_CAP": "7"},
              "host": {"MASH_AMD_HOST_FINISH": "1"}}


def mash(args, cwd, extra_env):
    env = dict(os.environ)
    for k in ("MASH_AMD_HOST_FINISH", "MASHGPU_RESULTS_MATRIX", "MASHGPU_CLUSTER_BLOCK_PAIRS", "MASHGPU_FOREST_EDGE_CAP", "MASHGPU_GREEDY_EDGE_CAP"):
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
    want = fm.forest_stdout_of_triangle(texts[name], cases["names"])
    assert want and want != texts[name]
    args = ["cluster", "-T", *cases["sketch"], *cluster_options(c["options"]), cases["input"]]
    errs = set()
    for route, env in CLI_ROUTES.items():
        r = mash(args, GOLD, env)
        assert r.stdout == want, (name, route)
        errs.add(r.stderr)
    assert len(errs) == 1


def test_command_with_comments_and_without_t():
    cases, texts = recorded()
    for name in ("d2", "dv"):
        opts = cluster_options([c["options"] for c in cases["cases"] if c["name"] == name][0])
        want_c = fm.forest_stdout_of_triangle(texts[name], cases["names"], cases["comments"])
        for route in ("lists", "matrix in blocks of 100 pairs", "host"):
            r = mash(["cluster", "-T", "-C", *cases["sketch"], *opts, cases["input"]], GOLD, CLI_ROUTES[route])
            assert r.stdout == want_c, (name, route)
        # without -T nothing has changed
        r = mash(["cluster", *cases["sketch"], *opts, cases["input"]], GOLD, {})
        assert r.stdout == cm.cluster_stdout_of_triangle(texts[name], cases["names"])
        r = mash(["cluster", "-R", *cases["sketch"], *opts, cases["input"]], GOLD, {})
        assert r.stdout == gm.greedy_stdout_of_triangle(texts[name], cases["names"])


def test_command_default_distance_is_0_05():
    cases, texts = recorded()
    want = fm.forest_stdout_of_triangle(texts["d3"], cases["names"])
    for env in ({}, {"MASH_AMD_HOST_FINISH": "1"}):
        assert mash(["cluster", "-T", *cases["sketch"], cases["input"]], GOLD, env).stdout == want


# ------------------------------------------------------------------------------------------ through the C ABI

def with_options(eng, opts, fn):
    for o, v in opts.items():
        eng.set_option(o, v)
    try:
        return fn()
    finally:
        for o in opts:
            eng.set_option(o, None)


def log2_floor(n):
    return max(n, 1).bit_length() - 1


def check_table(eng, t, n, filters, routes=ROUTES, k=21, kspace=KSPACE21, capacity=1 << 22):
    """the forest of every filter on every route against the model over mg_compare_tri_results_host's records, the labels and counts
    against mg_cluster_tri_host; -> {filter: (forest records, all records, {route: stats})}"""
    out = {}
    for fname, (max_d, max_p) in filters.items():
        rec = eng.compare_tri_results(t, k, kspace, max_d, max_p, capacity=capacity)
        assert np.all(rec["col"] < rec["row"])
        want = rec[fm.forest_fast(n, rec["row"], rec["col"], rec["numer"], rec["denom"])]
        lab, nc_single, ne_single = eng.cluster_tri_host(t, k, kspace, max_d, max_p)
        assert ne_single == len(rec) and len(want) == n - nc_single
        stats = {}
        for route, opts in routes.items():
            got, label, nc, ne = with_options(eng, opts, lambda: eng.cluster_tri_forest_host(t, k, kspace, max_d, max_p))
            st = eng.cluster_forest_stats()
            print(f"n {n} filter {fname} route {route}: edges {ne} clusters {nc} forest {len(got)} {st}")
            assert ne == len(rec), (fname, route, ne, len(rec))
            assert nc == nc_single and np.array_equal(label, lab), (fname, route)
            assert len(got) == n - nc, (fname, route, len(got))
            for f in ("row", "col", "numer", "denom"):
                assert np.array_equal(got[f], want[f]), (fname, route, f, int((got[f] != want[f]).sum()))
            assert got.tobytes() == want.tobytes(), (fname, route)                 # the doubles bit for bit
            live, chosen = eng.cluster_forest_rounds()
            if ne:
                assert 1 <= st["rounds"] <= log2_floor(n) + 1 and st["edge_capacity"] >= ne, (fname, route, st)
                assert len(live) == st["rounds"] and live[0] == ne and chosen[-1] == 0 and sum(chosen) == len(got), (fname, route, live, chosen)
                assert all(a > b for a, b in zip(live, live[1:])) and all(c >= 1 for c in chosen[:-1]), (fname, route, live, chosen)
            else:
                assert st["rounds"] == 0 and live == [] and chosen == []
            forced = "MASHGPU_FOREST_EDGE_CAP" in opts and ne > int(opts["MASHGPU_FOREST_EDGE_CAP"])
            assert (st["regrows"] >= 1) == forced, (fname, route, st)   # regrown exactly where the first capacity forces it
            stats[route] = st
        out[fname] = (want, rec, stats)
    return out


def test_c3_style_table_every_route(eng):
    n = 20000
    table, nh, lengths = synth.clustered_sketches(n, 1000, clusters=n // 100, seed=3)
    t = eng.table_upload(table, nh, lengths)
    res = check_table(eng, t, n, {"d": (0.05, -1.0), "both": (0.05, 1e-10)})
    forest, rec, stats = res["d"]
    assert 0 < len(forest) < len(rec) < n * (n - 1) // 2                   # the filter bites, and most edges are no forest edges
    assert stats["short list"]["regrows"] >= 1 and stats["default"]["regrows"] == 0
    t.free()


def test_one_species_millions_of_edges_and_runs_of_equal_fractions(eng):
    n = 4096
    table, nh, lengths = synth.species_sketches(n, 1000, seed=1)
    t = eng.table_upload(table, nh, lengths)
    res = check_table(eng, t, n, {"d": (0.05, -1.0), "v": (-1.0, 1e-10)}, capacity=1 << 23)
    assert len(res["v"][1]) > 8_000_000 and len(res["d"][1]) > 500_000   # -v alone passes nearly every pair, -d every tenth
    forest, rec, _ = res["d"]
    _, counts = np.unique(forest["numer"], return_counts=True)            # (one denominator here: equal numerators are equal fractions)
    assert np.all(forest["denom"] == 1000) and counts.max() >= 5
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


def test_path_and_band_in_index_order_take_13_rounds_at_most(eng):
    n, s, step = 5000, 1000, 100
    table, nh, lengths = window_table(n, s, step, seed=5)
    t = eng.table_upload(table, nh, lengths)
    d = [mash_distance(s - k * step, s) for k in range(6)]
    path_d, band_d = (d[1] + d[2]) / 2, (d[3] + d[4]) / 2           # edges (i, i + 1) alone; edges (i, i + k), k <= 3
    routes = {r: ROUTES[r] for r in ("default", "matrix", "blocks, short list")}
    res = check_table(eng, t, n, {"path": (path_d, -1.0), "band": (band_d, -1.0)}, routes=routes)
    forest, rec, stats = res["path"]
    assert len(rec) == n - 1 and len(forest) == n - 1                # every fraction equal: the forest is the path, in index order
    assert np.array_equal(forest["row"], np.arange(1, n)) and np.array_equal(forest["col"], np.arange(n - 1))
    for route, st in stats.items():
        assert 2 <= st["rounds"] <= 13, (route, st)                  # the greedy rounds need n / 2 here
    forest, rec, stats = res["band"]
    assert len(rec) == 3 * n - 6 and len(forest) == n - 1
    assert np.array_equal(forest["row"], np.arange(1, n)) and np.array_equal(forest["col"], np.arange(n - 1)) and np.all(forest["numer"] == s - step)
    for route, st in stats.items():
        assert 2 <= st["rounds"] <= 13, (route, st)
    t.free()


def ragged_table(n=2000, s=200, seed=11):
    """one species of n rows, every third row cut to its first 50 or 100 hashes: a pair of two cut rows has fewer than s union
    elements, so its denominator is the size of that union -- x shared strata of T give x / (2 T - x)"""
    table, nh, lengths = synth.species_sketches(n, s, seed=seed)
    nh = nh.copy()
    for i in range(0, n, 3):
        nh[i] = 50 if i % 2 else 100
        table[i, nh[i]:] = PAD
    return table, nh, lengths


def test_ragged_rows_many_denominators(eng):
    n = 2000
    table, nh, lengths = ragged_table(n)
    assert int((nh < 200).sum()) == (n + 2) // 3
    t = eng.table_upload(table, nh, lengths)
    res = check_table(eng, t, n, {"d": (0.05, -1.0)})
    forest, rec, _ = res["d"]
    assert len(set(rec["denom"].tolist())) >= 3                      # the passing edges carry at least three distinct denominators
    by_value = {}
    for numer, denom in set(zip(rec["numer"].tolist(), rec["denom"].tolist())):
        by_value.setdefault(Fraction(numer, denom), set()).add(denom)
    assert any(len(d) >= 2 for d in by_value.values())               # ... and some fraction value occurs under two of them
    assert len(set(forest["denom"].tolist())) >= 3
    t.free()


def test_block_boundaries_and_list_sizes(eng):
    """the matrix route in row blocks of one pair, of a few rows and in one block; first capacities of 1 edge, of a few, of one short
    and of exactly the number of edges"""
    n = 1200
    table, nh, lengths = synth.species_sketches(n, 1000, seed=7)
    t = eng.table_upload(table, nh, lengths)
    ne = len(eng.compare_tri_results(t, 21, KSPACE21, 0.05, -1.0, capacity=1 << 22))
    routes = {f"blocks of {b} pairs": {"MASHGPU_RESULTS_MATRIX": "1", "MASHGPU_CLUSTER_BLOCK_PAIRS": str(b)} for b in (1, 4097, 1 << 30)}
    routes.update({f"a list of {c} edges at first": {"MASHGPU_FOREST_EDGE_CAP": str(c)} for c in (1, 63, ne - 1, ne)})
    routes["blocks of 4097 pairs, a list of 1 edge"] = {"MASHGPU_RESULTS_MATRIX": "1", "MASHGPU_CLUSTER_BLOCK_PAIRS": "4097", "MASHGPU_FOREST_EDGE_CAP": "1"}
    res = check_table(eng, t, n, {"d": (0.05, -1.0)}, routes=routes)
    stats = res["d"][2]
    assert ne > 64 and stats[f"a list of {ne} edges at first"]["regrows"] == 0 and stats[f"a list of {ne - 1} edges at first"]["regrows"] == 1
    t.free()


# ------------------------------------------------------------------------------------------ calling conventions

def test_repeated_calls_capacity_and_no_labels(eng):
    n = 4096
    table, nh, lengths = synth.species_sketches(n, 1000, seed=4)
    t = eng.table_upload(table, nh, lengths)
    for route, opts in ROUTES.items():
        first = with_options(eng, opts, lambda: eng.cluster_tri_forest_host(t, 21, KSPACE21, 0.03, -1.0))
        again = with_options(eng, opts, lambda: eng.cluster_tri_forest_host(t, 21, KSPACE21, 0.03, -1.0))
        assert again[0].tobytes() == first[0].tobytes() and np.array_equal(again[1], first[1]) and again[2:] == first[2:], route
    count = len(first[0])
    assert count > 1
    # one record short: MG_ERR_NOMEM, the count, the labels and the counts -- and the context still works
    out = np.zeros(count, dtype=abi.RESULT_DTYPE)
    label = np.zeros(n, dtype=np.uint32)
    cnt, nc, ne = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    rc = eng.lib.mg_cluster_tri_forest_host(eng.ctx, t.handle, 21, KSPACE21, 0.03, -1.0, out.ctypes.data, count - 1, C.byref(cnt), label.ctypes.data,
                                            C.byref(nc), C.byref(ne))
    assert rc == MG_ERR_NOMEM and cnt.value == count and (nc.value, ne.value) == first[2:] and np.array_equal(label, first[1])
    rc = eng.lib.mg_cluster_tri_forest_host(eng.ctx, t.handle, 21, KSPACE21, 0.03, -1.0, out.ctypes.data, count, C.byref(cnt), None, C.byref(nc), C.byref(ne))
    assert rc == abi.MG_OK and cnt.value == count and out.tobytes() == first[0].tobytes()        # label_out_host == NULL
    got, label, _, _ = eng.cluster_tri_forest_host(t, 21, KSPACE21, 0.03, -1.0, want_label=False)
    assert label is None and got.tobytes() == first[0].tobytes()
    t.free()


def test_tables_of_no_and_one_row(eng):
    one = np.sort(np.random.default_rng(1).integers(0, 1 << 54, (1, 64), dtype=np.uint64), axis=1)
    t = eng.table_upload(one, np.full(1, 64, dtype=np.uint32), np.full(1, 1000, dtype=np.uint64))
    got, label, nc, ne = eng.cluster_tri_forest_host(t, 21, KSPACE21, 0.05, -1.0)
    assert len(got) == 0 and list(label) == [0] and (nc, ne) == (1, 0)
    t.free()
    t = eng.table_upload(np.zeros((0, 64), dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint64))
    got, label, nc, ne = eng.cluster_tri_forest_host(t, 21, KSPACE21, 0.05, -1.0)
    assert len(got) == 0 and len(label) == 0 and (nc, ne) == (0, 0)
    t.free()


def test_error_returns(eng):
    table, nh, lengths = synth.clustered_sketches(96, 1000, clusters=3, seed=1)
    t = eng.table_upload(table, nh, lengths)
    out = np.zeros(96, dtype=abi.RESULT_DTYPE)
    label = np.zeros(96, dtype=np.uint32)
    cnt, nc, ne = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)

    def call(max_d, max_p, k=21, out_ptr=out.ctypes.data, cnt_ref=C.byref(cnt)):
        return eng.lib.mg_cluster_tri_forest_host(eng.ctx, t.handle, k, KSPACE21, max_d, max_p, out_ptr, 96, cnt_ref, label.ctypes.data, C.byref(nc), C.byref(ne))

    for max_d, max_p in ((-1.0, -1.0), (1.0, 1.0), (1.0, -1.0), (2.0, 1.5)):
        assert call(max_d, max_p) == MG_ERR_INVALID
        assert b"both filters are off" in eng.lib.mg_last_error(eng.ctx)
    assert call(0.05, -1.0, out_ptr=None) == MG_ERR_INVALID
    assert call(0.05, -1.0, cnt_ref=None) == MG_ERR_INVALID
    assert call(0.05, -1.0, k=0) == MG_ERR_INVALID
    assert call(0.05, -1.0) == abi.MG_OK and int(nc.value) == 3 and int(cnt.value) == 93      # the context still works
    t.free()
