"""`mash cluster -L` and mg_cluster_tri_complete_host / _dev on the device.

Through the command: for every recorded case of tests/golden/cluster (stdout of the REFERENCE CLI's `triangle -E`) the command
prints, byte for byte, what tests/complete_model.py makes of the recorded stdout -- on the candidate-list route, with the matrix
route forced, with the matrix in row blocks of 100 pairs, with an edge list of 7 edges at first, with first batches of one round
(MASHGPU_COMPLETE_BATCH=1), and on the host route (MASH_AMD_HOST_FINISH=1); the same with -C; the default -d is 0.05; `mash cluster`
and `mash cluster -R` print what they printed before.
Through the C ABI: the labels against the model over the records of mg_compare_tri_results_host (the existing, oracle-verified
call), every cluster a clique of those records and no two clusters linked, n_edges and the regrow count equal to
mg_cluster_tri_forest_host's on the same table and options, on every route, with a short first list and with batches of one round:
a clade table of 2 000 rows in 20 clusters, one species of 1 000 rows (long runs of equal fractions), a ragged
table whose edges carry many denominators; the _dev form with a guard word; tables of 0 and 1 rows; a sketch size of 2^21 and both
filters off are refused.
Here, and only here, workgroups race on best_key / best_rc and on the lookup's slots: the emulator (tests/test_complete_emu.py) runs
them one after another.  Every command runs under its own timeout."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from mash_amd import abi
from tests import cluster_greedy_model as gm
from tests import cluster_model as cm
from tests import complete_model as lm
from workloads import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASH = os.path.join(ROOT, "mash_amd", "bin", "mash")
GOLD = os.path.join(ROOT, "tests", "golden", "cluster")
KSPACE21 = 4.0 ** 21
MG_ERR_INVALID, MG_ERR_UNSUPPORTED = -1, -2          # include/mashgpu.h
PAD = np.uint64(0xFFFFFFFFFFFFFFFF)
COUNTS = {"d1": 33, "d2": 24, "d3": 9, "v": 7, "dv": 8}

ROUTES = {"default": {}, "matrix": {"MASHGPU_RESULTS_MATRIX": "1"},
          "blocks": {"MASHGPU_RESULTS_MATRIX": "1", "MASHGPU_CLUSTER_BLOCK_PAIRS": "200000"},
          "short list": {"MASHGPU_FOREST_EDGE_CAP": "1000"},
          "batches from one round": {"MASHGPU_COMPLETE_BATCH": "1"},
          "blocks, short list, batches from 3": {"MASHGPU_RESULTS_MATRIX": "1", "MASHGPU_CLUSTER_BLOCK_PAIRS": "200000", "MASHGPU_FOREST_EDGE_CAP": "1000",
                                                 "MASHGPU_COMPLETE_BATCH": "3"}}


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
              "batches from one round": {"MASHGPU_COMPLETE_BATCH": "1"},
              "blocks, a short list and batches from one round": {"MASHGPU_RESULTS_MATRIX": "1", "MASHGPU_CLUSTER_BLOCK_PAIRS": "100",
                                                                  "MASHGPU_FOREST_EDGE_CAP": "7", "MASHGPU_COMPLETE_BATCH": "1"},
              "host": {"MASH_AMD_HOST_FINISH": "1"}}


def mash(args, cwd, extra_env):
    env = dict(os.environ)
    for k in ("MASH_AMD_HOST_FINISH", "MASHGPU_RESULTS_MATRIX", "MASHGPU_CLUSTER_BLOCK_PAIRS", "MASHGPU_FOREST_EDGE_CAP", "MASHGPU_GREEDY_EDGE_CAP",
              "MASHGPU_COMPLETE_BATCH"):
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


@pytest.mark.parametrize("name", sorted(COUNTS))
def test_command_on_the_recorded_family_every_route(name):
    cases, texts = recorded()
    c = [x for x in cases["cases"] if x["name"] == name][0]
    want = lm.complete_stdout_of_triangle(texts[name], cases["names"])
    assert len({ln.split("\t")[0] for ln in want.splitlines()}) == COUNTS[name]
    assert want != cm.cluster_stdout_of_triangle(texts[name], cases["names"])          # not the single-linkage partition
    args = ["cluster", "-L", *cases["sketch"], *cluster_options(c["options"]), cases["input"]]
    errs = set()
    for route, env in CLI_ROUTES.items():
        r = mash(args, GOLD, env)
        assert r.stdout == want, (name, route)
        errs.add(r.stderr)
    assert len(errs) == 1


def test_command_with_comments_and_without_l():
    cases, texts = recorded()
    for name in ("d2", "dv"):
        opts = cluster_options([c["options"] for c in cases["cases"] if c["name"] == name][0])
        want_c = lm.complete_stdout_of_triangle(texts[name], cases["names"], cases["comments"])
        for route in ("lists", "matrix in blocks of 100 pairs", "host"):
            r = mash(["cluster", "-L", "-C", *cases["sketch"], *opts, cases["input"]], GOLD, CLI_ROUTES[route])
            assert r.stdout == want_c, (name, route)
        # without -L nothing has changed
        r = mash(["cluster", *cases["sketch"], *opts, cases["input"]], GOLD, {})
        assert r.stdout == cm.cluster_stdout_of_triangle(texts[name], cases["names"])
        r = mash(["cluster", "-R", *cases["sketch"], *opts, cases["input"]], GOLD, {})
        assert r.stdout == gm.greedy_stdout_of_triangle(texts[name], cases["names"])


def test_command_default_distance_is_0_05():
    cases, texts = recorded()
    want = lm.complete_stdout_of_triangle(texts["d3"], cases["names"])
    for env in ({}, {"MASH_AMD_HOST_FINISH": "1"}):
        assert mash(["cluster", "-L", *cases["sketch"], cases["input"]], GOLD, env).stdout == want


# ------------------------------------------------------------------------------------------ through the C ABI

def with_options(eng, opts, fn):
    for o, v in opts.items():
        eng.set_option(o, v)
    try:
        return fn()
    finally:
        for o in opts:
            eng.set_option(o, None)


def check_table(eng, t, n, max_d, max_p, routes=ROUTES, k=21, kspace=KSPACE21, capacity=1 << 22):
    """the labels of every route against the model over mg_compare_tri_results_host's records; -> (records, labels, {route: stats})"""
    rec = eng.compare_tri_results(t, k, kspace, max_d, max_p, capacity=capacity)
    assert np.all(rec["col"] < rec["row"])
    want = np.array(lm.walk_fast(n, rec["row"], rec["col"], rec["numer"], rec["denom"]), dtype=np.uint32)
    edges = list(zip(rec["row"].tolist(), rec["col"].tolist()))
    assert cm.non_clique_clusters(want.tolist(), edges) == [] and lm.linked_pairs(want.tolist(), edges) == []
    stats = {}
    for route, opts in routes.items():
        forest_opts = {o: v for o, v in opts.items() if o != "MASHGPU_COMPLETE_BATCH"}
        _, _, _, ne_forest = with_options(eng, forest_opts, lambda: eng.cluster_tri_forest_host(t, k, kspace, max_d, max_p))
        forest_regrows = eng.cluster_forest_stats()["regrows"]
        label, nc, ne = with_options(eng, opts, lambda: eng.cluster_tri_complete_host(t, k, kspace, max_d, max_p))
        st = eng.cluster_complete_stats()
        live, merged = eng.cluster_complete_rounds()
        print(f"n {n} route {route}: edges {ne} clusters {nc} {st} merged per round {merged[:12]}")
        assert ne == len(rec) == ne_forest and st["regrows"] == forest_regrows, (route, ne, len(rec), ne_forest, st)
        bad = np.flatnonzero(label != want)
        assert len(bad) == 0, (route, len(bad), bad[:10], label[bad[:10]], want[bad[:10]])
        assert nc == len(set(want.tolist())), (route, nc)
        assert cm.non_clique_clusters(label.tolist(), edges) == [], route
        if ne:
            assert 2 <= st["rounds"] <= n and st["edge_capacity"] >= ne and len(live) == st["rounds"], (route, st)
            assert live[0] == ne and live[-1] == 0 and merged[-1] == 0 and sum(merged) == n - nc, (route, live[:5], merged[:5])
            assert all(a > b for a, b in zip(live, live[1:])) and all(m >= 1 for m in merged[:-1]), route
            first = int(opts.get("MASHGPU_COMPLETE_BATCH", 8))
            sizes, total = 0, 0
            while total < st["rounds"]:
                total += min(first << sizes, 256)
                sizes += 1
            assert st["batches"] == sizes, (route, st, first)
        else:
            assert st["rounds"] == 0 and st["batches"] == 0 and live == []
        stats[route] = st
    return rec, want, stats


def test_clade_table_every_route(eng):
    n = 2000
    table, nh, lengths = synth.clustered_sketches(n, 1000, clusters=20, seed=3)
    t = eng.table_upload(table, nh, lengths)
    rec, want, stats = check_table(eng, t, n, 0.05, -1.0)
    assert len(rec) > 10 * n and 20 <= len(set(want.tolist())) < n            # clusters inside the clades, never across them
    assert all(want[i] % 20 == i % 20 for i in range(n))
    assert stats["short list"]["regrows"] >= 1 and stats["default"]["regrows"] == 0
    both, _, _ = check_table(eng, t, n, 0.05, 1e-10, routes={r: ROUTES[r] for r in ("default", "blocks, short list, batches from 3")})
    assert len(both) <= len(rec)
    t.free()


def test_one_species_long_runs_of_equal_fractions(eng):
    n = 1000
    table, nh, lengths = synth.species_sketches(n, 1000, seed=1)
    t = eng.table_upload(table, nh, lengths)
    rec, want, stats = check_table(eng, t, n, 0.05, -1.0)
    _, counts = np.unique(rec["numer"], return_counts=True)                   # (one denominator here: equal numerators are equal fractions)
    assert np.all(rec["denom"] == 1000) and counts.max() >= 50 and len(rec) > 10 * n
    single = cm.labels_fast(n, rec["row"], rec["col"])
    assert len(set(single)) < len(set(want.tolist()))                         # single linkage chains here; complete linkage does not
    t.free()


def ragged_table(n=1200, s=200, seed=11):
    """one species of n rows, every third row cut to its first 50 or 100 hashes: a pair of two cut rows has fewer than s union
    elements, so its denominator is the size of that union"""
    table, nh, lengths = synth.species_sketches(n, s, seed=seed)
    nh = nh.copy()
    for i in range(0, n, 3):
        nh[i] = 50 if i % 2 else 100
        table[i, nh[i]:] = PAD
    return table, nh, lengths


def test_ragged_rows_many_denominators(eng):
    n = 1200
    table, nh, lengths = ragged_table(n)
    t = eng.table_upload(table, nh, lengths)
    rec, want, _ = check_table(eng, t, n, 0.05, -1.0, routes={r: ROUTES[r] for r in ("default", "matrix", "short list")})
    assert len(set(rec["denom"].tolist())) >= 3 and len(set(want.tolist())) < n
    t.free()


def test_dev_form_and_repeated_calls(eng):
    import torch
    n = 1000
    table, nh, lengths = synth.species_sketches(n, 1000, seed=4)
    t = eng.table_upload(table, nh, lengths)
    first = eng.cluster_tri_complete_host(t, 21, KSPACE21, 0.03, -1.0)
    assert first[1] < n
    for _ in range(2):
        d_lab = torch.full((n + 1,), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
        nc, ne = eng.cluster_tri_complete_dev(t, 21, KSPACE21, d_lab.data_ptr(), 0.03, -1.0)
        torch.cuda.synchronize()
        got = d_lab.cpu().numpy().view(np.uint32)
        assert got[n] == 0x7FFFFFFF and np.array_equal(got[:n], first[0]) and (nc, ne) == first[1:]
    again = eng.cluster_tri_complete_host(t, 21, KSPACE21, 0.03, -1.0)
    assert np.array_equal(again[0], first[0]) and again[1:] == first[1:]
    t.free()


def test_tables_of_no_and_one_row(eng):
    one = np.sort(np.random.default_rng(1).integers(0, 1 << 54, (1, 64), dtype=np.uint64), axis=1)
    t = eng.table_upload(one, np.full(1, 64, dtype=np.uint32), np.full(1, 1000, dtype=np.uint64))
    label, nc, ne = eng.cluster_tri_complete_host(t, 21, KSPACE21, 0.05, -1.0)
    assert list(label) == [0] and (nc, ne) == (1, 0) and eng.cluster_complete_stats()["rounds"] == 0
    t.free()
    t = eng.table_upload(np.zeros((0, 64), dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint64))
    label, nc, ne = eng.cluster_tri_complete_host(t, 21, KSPACE21, 0.05, -1.0)
    assert len(label) == 0 and (nc, ne) == (0, 0)
    t.free()


def test_error_returns(eng):
    table, nh, lengths = synth.clustered_sketches(96, 1000, clusters=3, seed=1)
    t = eng.table_upload(table, nh, lengths)
    label = np.zeros(96, dtype=np.uint32)
    nc, ne = C.c_uint64(0), C.c_uint64(0)

    def call(fn, max_d, max_p, k=21, table=t, out=label.ctypes.data, nc_ref=C.byref(nc)):
        return fn(eng.ctx, table.handle, k, KSPACE21, max_d, max_p, out, nc_ref, C.byref(ne))

    for fn in (eng.lib.mg_cluster_tri_complete_host, eng.lib.mg_cluster_tri_complete_dev):
        for max_d, max_p in ((-1.0, -1.0), (1.0, 1.0), (1.0, -1.0), (2.0, 1.5)):
            assert call(fn, max_d, max_p) == MG_ERR_INVALID
            assert b"both filters are off" in eng.lib.mg_last_error(eng.ctx)
        assert call(fn, 0.05, -1.0, out=None) == MG_ERR_INVALID
        assert call(fn, 0.05, -1.0, nc_ref=None) == MG_ERR_INVALID
    assert call(eng.lib.mg_cluster_tri_complete_host, 0.05, -1.0, k=0) == MG_ERR_INVALID
    # a sketch size of 2^21: the weight key is exact below that only
    s = 1 << 21
    wide = np.arange(1, 2 * s + 1, dtype=np.uint64).reshape(2, s)
    tw = eng.table_upload(wide, np.full(2, s, dtype=np.uint32), np.full(2, 5_000_000, dtype=np.uint64))
    assert call(eng.lib.mg_cluster_tri_complete_host, 0.05, -1.0, table=tw) == MG_ERR_UNSUPPORTED
    assert b"2^21" in eng.lib.mg_last_error(eng.ctx)
    tw.free()
    assert call(eng.lib.mg_cluster_tri_complete_host, 0.05, -1.0) == abi.MG_OK and 3 <= int(nc.value) < 96      # the context still works
    assert np.array_equal(label % 3, np.arange(96, dtype=np.uint32) % 3) and np.all(label[label] == label)
    t.free()
