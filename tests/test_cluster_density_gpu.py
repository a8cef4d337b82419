"""`mash cluster -D` and mg_cluster_tri_density_host / mg_cluster_tri_density_dev on the device.

1. Through the command: for six (case, m) pairs of tests/golden/cluster (stdout of the REFERENCE CLI's `triangle -E`) and m = 1 on d2
   the command prints, byte for byte, what tests/cluster_density_model.py makes of the recorded stdout -- on the candidate-list route,
   with the matrix route forced, with the matrix in row blocks of 100 pairs, with an edge list of 7 edges at first, with both, and on
   the host route (MASH_AMD_HOST_FINISH=1); stderr is the same on every route; the same with -C; at m = 1 the first three fields are
   plain `mash cluster`'s stdout.
2. A bridge table whose answer has a closed form: three groups A, B, C of 60 rows, a bridge row between A and B that is nearer the
   LATER group and precedes every row of both, a bridge row between B and C with an exact tie, and a row apart.  Single linkage
   chains A, B and C; -D 30 does not.
3. One species of 1 200 rows against the model over mg_compare_tri_results_host's records, in blocks and with short lists.
4. Calling conventions: the _dev form with guard words, NULL via / degree, repeated calls, 0 and 1 rows, the error returns.
Here, and only here, workgroups race on deg[], parent[], best_key[] and via[]: the emulator (tests/test_cluster_density_emu.py) runs
them one after another.  Every command runs under its own timeout; a non-zero exit ends the test.  The MG_ERR_UNSUPPORTED return for
a sketch size of 2^21 or more is not exercised (it would need a table of that width); it is one comparison in cluster_jobs
(host_cluster.cpp)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from mash_amd import abi
from tests import cluster_density_model as dm
from tests import cluster_model as cm
from workloads import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASH = os.path.join(ROOT, "mash_amd", "bin", "mash")
GOLD = os.path.join(ROOT, "tests", "golden", "cluster")
KSPACE21 = 4.0 ** 21
MG_ERR_INVALID = -1             # include/mashgpu.h


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
    for k in ("MASH_AMD_HOST_FINISH", "MASHGPU_RESULTS_MATRIX", "MASHGPU_CLUSTER_BLOCK_PAIRS", "MASHGPU_GREEDY_EDGE_CAP", "MASHGPU_DENSITY_PLAIN"):
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


def first_three(text):
    return "".join("\t".join(ln.split("\t")[:3]) + "\n" for ln in text.splitlines())


@pytest.mark.parametrize("name,m", [("d1", 3), ("d2", 3), ("d2", 6), ("d3", 10), ("v", 38), ("dv", 35), ("d2", 1)])
def test_command_on_the_recorded_family_every_route(name, m):
    cases, texts = recorded()
    c = [x for x in cases["cases"] if x["name"] == name][0]
    want = dm.density_stdout_of_triangle(texts[name], cases["names"], m)
    plain = cm.cluster_stdout_of_triangle(texts[name], cases["names"])
    if m > 1:
        assert "\tborder\t" in want and "\tcore\t" in want and "\tnoise\t" in want
    args = [*cases["sketch"], *cluster_options(c["options"]), cases["input"]]
    errs = set()
    for route, env in CLI_ROUTES.items():
        r = mash(["cluster", "-D", str(m), *args], GOLD, env)
        assert r.stdout == want, (name, m, route)
        errs.add(r.stderr)
    assert len(errs) == 1
    if m == 1:
        assert first_three(want) == plain and mash(["cluster", *args], GOLD, {}).stdout == plain
        assert mash(["cluster", "-D", "1", *args], GOLD, {"MASHGPU_DENSITY_PLAIN": "1"}).stdout == want
    elif name in ("d1", "d2", "d3"):
        assert first_three(want) != plain                          # the partition is not single linkage's


def test_command_with_comments():
    cases, texts = recorded()
    for name, m in (("d2", 6), ("dv", 35)):
        opts = cluster_options([c["options"] for c in cases["cases"] if c["name"] == name][0])
        want_c = dm.density_stdout_of_triangle(texts[name], cases["names"], m, cases["comments"])
        for route in ("lists", "matrix in blocks of 100 pairs", "host"):
            r = mash(["cluster", "-D", str(m), "-C", *cases["sketch"], *opts, cases["input"]], GOLD, CLI_ROUTES[route])
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


def offset_table(offsets, s, seed):
    """row i is the window pool[offsets[i] : offsets[i] + s] of one ascending pool of distinct hashes: two rows whose offsets differ by
    k < s share s - k of the s smallest values of their union"""
    rng = np.random.default_rng(seed)
    need = int(max(offsets)) + s
    pool = np.unique(rng.integers(0, 1 << 54, need + need // 8 + 64, dtype=np.uint64))[:need]
    assert len(pool) == need
    idx = np.asarray(offsets, dtype=np.int64)[:, None] + np.arange(s, dtype=np.int64)[None, :]
    n = len(offsets)
    return pool[idx], np.full(n, s, dtype=np.uint32), np.full(n, 1_000_000, dtype=np.uint64)


def mash_distance(shared, s, k=21):
    j = shared / s
    return -np.log(2 * j / (1 + j)) / k


def model_of_records(n, rec, m):
    label, via, deg = dm.density_fast(n, rec["row"], rec["col"], rec["numer"], rec["denom"], m)
    return np.array(label, dtype=np.uint32), np.array(via, dtype=np.uint32), np.array(deg, dtype=np.uint32)


def test_bridge_table_with_a_closed_form(eng):
    s = 1000
    offsets = [890] + list(range(0, 600, 10)) + list(range(1140, 1740, 10)) + [2030] + list(range(2330, 2930, 10)) + [20000]
    n = len(offsets)
    assert n == 183 and offsets[61] == 1140 and offsets[120] == 1730 and offsets[122] == 2330
    table, nh, lengths = offset_table(offsets, s, seed=11)
    t = eng.table_upload(table, nh, lengths)
    max_d = (mash_distance(650, s) + mash_distance(640, s)) / 2
    rec = eng.compare_tri_results(t, 21, KSPACE21, max_d, -1.0)
    off = np.asarray(offsets)
    apart = np.abs(off[rec["row"]] - off[rec["col"]])
    assert len(rec) == 4439 and (apart <= 350).all() and (rec["denom"] == s).all() and np.array_equal(rec["numer"], s - apart)
    want_deg = np.array([int((np.abs(off - o) <= 350).sum()) - 1 for o in off], dtype=np.uint32)
    assert want_deg[0] == 17 and want_deg[121] == 12 and want_deg[182] == 0 and want_deg[1:61].min() >= 35 and want_deg[61:121].min() >= 35
    assert want_deg[122:182].min() >= 35 and want_deg.max() < 70
    ident = np.arange(n, dtype=np.uint32)
    routes = {"default": {}, "plain degrees": {"MASHGPU_DENSITY_PLAIN": "1"}, "matrix": {"MASHGPU_RESULTS_MATRIX": "1"},
              "blocks of 4097 pairs, a list of 1 edge": {"MASHGPU_RESULTS_MATRIX": "1", "MASHGPU_CLUSTER_BLOCK_PAIRS": "4097", "MASHGPU_GREEDY_EDGE_CAP": "1"}}
    single, nc_single, ne_single = eng.cluster_tri_host(t, 21, KSPACE21, max_d, -1.0)
    assert (nc_single, ne_single) == (2, 4439)                       # single linkage chains A, B and C through the bridges
    for route, opts in routes.items():
        for m in (30, 1, 13, 17, 70):
            label, via, deg, nc, ne = with_options(eng, opts, lambda: eng.cluster_tri_density_host(t, 21, KSPACE21, m, max_d, -1.0))
            st = eng.cluster_density_stats()
            print(f"bridge route {route} m {m}: edges {ne} clusters {nc} {st}")
            w_label, w_via, w_deg = model_of_records(n, rec, m)
            assert ne == 4439 and np.array_equal(deg, want_deg) and np.array_equal(deg, w_deg), (route, m)
            assert np.array_equal(label, w_label) and np.array_equal(via, w_via) and nc == int((w_label == ident).sum()), (route, m)
            if m == 30:
                assert (nc, st["cores"], st["borders"], st["noise"]) == (4, 180, 2, 1), route
                assert via[0] == 61 and via[121] == 120 and np.array_equal(np.delete(via, [0, 121]), np.delete(ident, [0, 121])), route
                assert (label[1:61] == 1).all() and (label[61:122] == 0).all() and label[0] == 0 and (label[122:182] == 122).all() and label[182] == 182
            elif m == 1:
                assert nc == 2 and np.array_equal(label, single) and np.array_equal(via, ident) and st["borders"] == 0, route
            elif m in (13, 17):
                assert nc == 3 and st["cores"] == 181 and via[121] == 120 and label[0] == label[1] == label[61] == label[121] == 0, (route, m)
            else:
                assert nc == n and st["noise"] == n and np.array_equal(label, ident) and np.array_equal(via, ident), route
    t.free()


@pytest.fixture(scope="module")
def species(eng):
    n = 1200
    table, nh, lengths = synth.species_sketches(n, 1000, seed=7)
    t = eng.table_upload(table, nh, lengths)
    recs = {d: eng.compare_tri_results(t, 21, KSPACE21, d, -1.0, capacity=1 << 22) for d in (0.03, 0.05)}
    yield n, t, recs
    t.free()


@pytest.mark.parametrize("max_d,m", [(0.03, 10), (0.05, 200), (0.05, 400)])
def test_one_species_blocks_and_list_sizes(eng, species, max_d, m):
    """3. label, via, degree, clusters and edges against the model over mg_compare_tri_results_host's records; the matrix route in row
    blocks of one pair, of 4097 and in one block; first capacities of 1 edge, 63, one short and exactly enough.  What the model
    makes of the CPU oracle's pairs, for orientation (the test asserts the model's figures over the device's records, not these):
    d 0.03 m 10: 6 004 edges, 76 clusters, 607 cores, 579 borders, 14 noise; d 0.05: 200 072 edges, m 200: 1 cluster, 1011 / 189 / 0,
    m 400: 155 clusters, 325 / 721 / 154"""
    n, t, recs = species
    rec = recs[max_d]
    ne_want = len(rec)
    w_label, w_via, w_deg = model_of_records(n, rec, m)
    edges = list(zip(rec["row"].tolist(), rec["col"].tolist(), rec["numer"].tolist(), rec["denom"].tolist()))
    figures = dm.figures(w_label.tolist(), w_via.tolist(), w_deg.tolist(), m)
    first = dm.borders_first_in_their_cluster(w_label.tolist(), w_via.tolist(), w_deg.tolist(), m)
    print(f"species d {max_d} m {m}: edges {ne_want} (clusters, cores, borders, noise) {figures}, {len(first)} borders first in their cluster")
    assert ne_want > 64 and figures[2] > 0
    if (max_d, m) == (0.03, 10):
        ties = dm.borders_with_a_tie_for_best(w_via.tolist(), w_deg.tolist(), m, edges)
        print(f"    {len(ties)} borders with a tie for best")
        assert len(ties) > 0 and len(first) > 0
    routes = {f"blocks of {b} pairs": {"MASHGPU_RESULTS_MATRIX": "1", "MASHGPU_CLUSTER_BLOCK_PAIRS": str(b)} for b in (1, 4097, 1 << 30)}
    routes.update({f"a list of {c} edges at first": {"MASHGPU_GREEDY_EDGE_CAP": str(c)} for c in (1, 63, ne_want - 1, ne_want)})
    routes["plain degrees"] = {"MASHGPU_DENSITY_PLAIN": "1"}
    stats = {}
    for route, opts in routes.items():
        label, via, deg, nc, ne = with_options(eng, opts, lambda: eng.cluster_tri_density_host(t, 21, KSPACE21, m, max_d, -1.0))
        stats[route] = st = eng.cluster_density_stats()
        assert ne == ne_want, route
        assert np.array_equal(deg, w_deg), (route, int((deg != w_deg).sum()))
        assert np.array_equal(via, w_via), (route, int((via != w_via).sum()))
        assert np.array_equal(label, w_label), (route, int((label != w_label).sum()))
        assert (nc, st["cores"], st["borders"], st["noise"]) == figures and st["edge_capacity"] >= ne, (route, st)
    assert stats[f"a list of {ne_want} edges at first"]["regrows"] == 0 and stats[f"a list of {ne_want - 1} edges at first"]["regrows"] == 1
    assert stats["a list of 1 edges at first"]["regrows"] >= 1
    again = [eng.cluster_tri_density_host(t, 21, KSPACE21, m, max_d, -1.0) for _ in range(3)]      # three repeated calls, identical arrays
    for a in again:
        assert all(np.array_equal(x, y) for x, y in zip(a[:3], (w_label, w_via, w_deg))) and a[3:] == (figures[0], ne_want)


def test_one_neighbour_is_single_linkage(eng, species):
    n, t, recs = species
    for max_d in (0.03, 0.05):
        single = eng.cluster_tri_host(t, 21, KSPACE21, max_d, -1.0)
        label, via, deg, nc, ne = eng.cluster_tri_density_host(t, 21, KSPACE21, 1, max_d, -1.0)
        assert np.array_equal(label, single[0]) and (nc, ne) == single[1:] and np.array_equal(via, np.arange(n, dtype=np.uint32))
        assert ne == len(recs[max_d]) and int(deg.sum()) == 2 * ne


# ------------------------------------------------------------------------------------------ 4. calling conventions

def test_dev_form_and_null_outputs(eng, species):
    import torch
    n, t, recs = species
    want = eng.cluster_tri_density_host(t, 21, KSPACE21, 10, 0.03, -1.0)
    guard = 0x7FFFFFFF
    for _ in range(2):
        d = [torch.full((n + 1,), guard, dtype=torch.int32, device="cuda") for _ in range(3)]
        nc, ne = eng.cluster_tri_density_dev(t, 21, KSPACE21, 10, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 0.03, -1.0)
        torch.cuda.synchronize()
        for k in range(3):
            got = d[k].cpu().numpy().view(np.uint32)
            assert got[n] == guard and np.array_equal(got[:n], want[k]), k
        assert (nc, ne) == want[3:]
    d_label = torch.full((n + 1,), guard, dtype=torch.int32, device="cuda")
    assert eng.cluster_tri_density_dev(t, 21, KSPACE21, 10, d_label.data_ptr(), None, None, 0.03, -1.0) == want[3:]
    torch.cuda.synchronize()
    got = d_label.cpu().numpy().view(np.uint32)
    assert got[n] == guard and np.array_equal(got[:n], want[0])
    label = np.zeros(n, dtype=np.uint32)
    nc, ne = C.c_uint64(0), C.c_uint64(0)
    for via, deg in ((None, None), (np.zeros(n, dtype=np.uint32), None), (None, np.zeros(n, dtype=np.uint32))):
        rc = eng.lib.mg_cluster_tri_density_host(eng.ctx, t.handle, 21, KSPACE21, 0.03, -1.0, 10, label.ctypes.data, None if via is None else via.ctypes.data,
                                                 None if deg is None else deg.ctypes.data, C.byref(nc), C.byref(ne))
        assert rc == abi.MG_OK and np.array_equal(label, want[0]) and (int(nc.value), int(ne.value)) == want[3:]
        assert via is None or np.array_equal(via, want[1])
        assert deg is None or np.array_equal(deg, want[2])


def test_tables_of_no_and_one_row(eng):
    one = np.sort(np.random.default_rng(1).integers(0, 1 << 54, (1, 64), dtype=np.uint64), axis=1)
    t = eng.table_upload(one, np.full(1, 64, dtype=np.uint32), np.full(1, 1000, dtype=np.uint64))
    label, via, deg, nc, ne = eng.cluster_tri_density_host(t, 21, KSPACE21, 2, 0.05, -1.0)
    assert (list(label), list(via), list(deg), nc, ne) == ([0], [0], [0], 1, 0)
    assert eng.cluster_density_stats() == {"cores": 0, "borders": 0, "noise": 1, "regrows": 0, "edge_capacity": 0}
    t.free()
    t = eng.table_upload(np.zeros((0, 64), dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint64))
    label, via, deg, nc, ne = eng.cluster_tri_density_host(t, 21, KSPACE21, 2, 0.05, -1.0)
    assert len(label) == len(via) == len(deg) == 0 and (nc, ne) == (0, 0)
    t.free()


def test_error_returns(eng):
    table, nh, lengths = synth.clustered_sketches(96, 1000, clusters=3, seed=1)
    t = eng.table_upload(table, nh, lengths)
    bare = eng.table_upload(table, nh, None)
    out = [np.zeros(96, dtype=np.uint32) for _ in range(3)]
    nc, ne = C.c_uint64(0), C.c_uint64(0)

    def call(fn, max_d, max_p, m=3, k=21, table=t, label=out[0].ctypes.data, nc_ref=C.byref(nc)):
        return fn(eng.ctx, table.handle if table is not None else None, k, KSPACE21, max_d, max_p, m, label, out[1].ctypes.data, out[2].ctypes.data, nc_ref,
                  C.byref(ne))

    for fn in (eng.lib.mg_cluster_tri_density_host, eng.lib.mg_cluster_tri_density_dev):
        for max_d, max_p in ((-1.0, -1.0), (1.0, 1.0), (1.0, -1.0), (2.0, 1.5)):
            assert call(fn, max_d, max_p) == MG_ERR_INVALID
            assert b"both filters are off" in eng.lib.mg_last_error(eng.ctx)
        assert call(fn, 0.05, -1.0, m=0) == MG_ERR_INVALID and b"min_neighbours is 0" in eng.lib.mg_last_error(eng.ctx)
        assert call(fn, 0.05, -1.0, label=None) == MG_ERR_INVALID and b"NULL argument" in eng.lib.mg_last_error(eng.ctx)
        assert call(fn, 0.05, -1.0, table=None) == MG_ERR_INVALID
        assert call(fn, 0.05, -1.0, nc_ref=None) == MG_ERR_INVALID
        assert call(fn, 0.05, -1.0, table=bare) == MG_ERR_INVALID and b"no lengths" in eng.lib.mg_last_error(eng.ctx)
    assert call(eng.lib.mg_cluster_tri_density_host, 0.05, -1.0, k=0) == MG_ERR_INVALID
    assert call(eng.lib.mg_cluster_tri_density_host, 0.05, -1.0) == abi.MG_OK and int(nc.value) == 3      # the context still works
    bare.free()
    t.free()
