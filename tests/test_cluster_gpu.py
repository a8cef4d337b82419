"""`mash cluster` and mg_cluster_tri_host / mg_cluster_tri_dev on the device.

Through the command: for every recorded case of tests/golden/cluster (stdout of the REFERENCE CLI's `triangle -E`,
tests/golden/make_cluster_golden.py) the device route and the host route (MASH_AMD_HOST_FINISH=1) print exactly what
tests/cluster_model.py makes of the recorded stdout, with equal stderr; the same with -C, -l, -p 3 and .msh inputs.
Through the C ABI, on the candidate-list route and on the matrix route of the thresholded compare: labels, clusters and edges
against the model over the records of mg_compare_tri_results_host (the existing, oracle-verified call) on the same table; one
table against edges derived from the oracle's own distances and p-values.  Here, and only here, workgroups race on the parent
array: the emulator (tests/test_cluster_emu.py) runs them one after another."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from mash_amd import abi
from tests import cluster_model as cm
from workloads import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASH = os.path.join(ROOT, "mash_amd", "bin", "mash")
GOLD = os.path.join(ROOT, "tests", "golden", "cluster")
KSPACE21 = 4.0 ** 21
MG_ERR_INVALID = -1             # include/mashgpu.h

FILTERS = {"d": (0.05, -1.0), "v": (-1.0, 1e-10), "both": (0.05, 1e-10)}
# the two routes of the thresholded compare: the inverted-index engine's candidate lists, and row blocks of the matrix (the
# options the other result tests use to force them); "blocks": the matrix in row blocks of 2 000 000 pairs over one parent array
ROUTES = {"default": {}, "sparse": {"MASHGPU_COMPARE_KERNEL": "sparse"}, "matrix": {"MASHGPU_RESULTS_MATRIX": "1"},
          "blocks": {"MASHGPU_RESULTS_MATRIX": "1", "MASHGPU_CLUSTER_BLOCK_PAIRS": "2000000"}}


@pytest.fixture(scope="module")
def eng():
    import torch
    torch.cuda.init()          # (torch ships its own HIP runtime: it initialises first, tests/test_gpu_parity.py)
    e = abi.MashGpu(0)
    e.set_option("MASHGPU_COSTS_FIXED", "1")
    yield e
    e.close()


# ------------------------------------------------------------------------------------------ through the command

def mash(args, cwd, host_route):
    env = dict(os.environ)
    env.pop("MASH_AMD_HOST_FINISH", None)
    if host_route:
        env["MASH_AMD_HOST_FINISH"] = "1"
    r = subprocess.run([MASH, *args], cwd=cwd, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def cluster_options(triangle_options):
    """the options that make `mash cluster` use the filters of a recorded `mash triangle -E` run: triangle's -d defaults to 1,
    cluster's to 0.05, so a recording without -d is matched by an explicit -d 1"""
    return list(triangle_options) if "-d" in triangle_options else ["-d", "1", *triangle_options]


def recorded():
    cases = json.load(open(os.path.join(GOLD, "cases.json")))
    return cases, {c["name"]: open(os.path.join(GOLD, c["name"] + ".out")).read() for c in cases["cases"]}


def test_command_on_the_recorded_family_both_routes():
    cases, texts = recorded()
    seen = set()
    for c in cases["cases"]:
        want = cm.cluster_stdout_of_triangle(texts[c["name"]], cases["names"])
        seen.add(want)
        args = ["cluster", *cases["sketch"], *cluster_options(c["options"]), cases["input"]]
        dev, host = mash(args, GOLD, False), mash(args, GOLD, True)
        assert dev.stdout == want, (c["name"], "device route")
        assert host.stdout == want, (c["name"], "host route")
        assert dev.stderr == host.stderr
    assert len(seen) >= 4                                          # the cases do not all print the same thing


def test_command_default_distance_is_0_05():
    cases, texts = recorded()
    want = cm.cluster_stdout_of_triangle(texts["d3"], cases["names"])
    for host_route in (False, True):
        assert mash(["cluster", *cases["sketch"], cases["input"]], GOLD, host_route).stdout == want


def test_command_composes_with_comment_threads_list_and_sketch_files(tmp_path):
    cases, texts = recorded()
    fam = os.path.join(GOLD, cases["input"])
    sk = cases["sketch"]
    for name in ("d2", "dv"):
        opts = cluster_options([c["options"] for c in cases["cases"] if c["name"] == name][0])
        want = cm.cluster_stdout_of_triangle(texts[name], cases["names"])
        want_c = cm.cluster_stdout_of_triangle(texts[name], cases["names"], cases["comments"])
        lst = tmp_path / "in.txt"
        lst.write_text(fam + "\n")
        mash(["sketch", *sk, "-o", "fam", fam], str(tmp_path), False)
        for host_route in (False, True):
            outs = []
            for args, w in ((["-C", fam], want_c), (["-p", "3", fam], want), (["-l", str(lst)], want), (["-p", "3", "-C", "-l", str(lst)], want_c)):
                r = mash(["cluster", *sk, *opts, *args], str(tmp_path), host_route)
                assert r.stdout == w, (name, args, host_route)
                outs.append(r)
            r = mash(["cluster", *opts, "fam.msh"], str(tmp_path), host_route)
            assert r.stdout == want, (name, ".msh", host_route)
            r = mash(["cluster", "-C", *opts, "fam.msh"], str(tmp_path), host_route)
            assert r.stdout == want_c, (name, ".msh -C", host_route)


def test_command_stderr_is_the_same_on_both_routes_with_a_kmer_warning(tmp_path):
    """k = 8 on 2 500-base sequences draws the k-mer size warning `mash triangle` prints: both routes print it alike"""
    cases, _ = recorded()
    fam = os.path.join(GOLD, cases["input"])
    args = ["cluster", "-i", "-k", "8", "-s", "64", "-d", "0.2", fam]
    dev, host = mash(args, str(tmp_path), False), mash(args, str(tmp_path), True)
    tri = mash(["triangle", "-E", "-i", "-k", "8", "-s", "64", "-d", "0.2", fam], str(tmp_path), False)
    assert dev.stdout == host.stdout == cm.cluster_stdout_of_triangle(tri.stdout, cases["names"])
    assert dev.stderr == host.stderr == tri.stderr and "WARNING" in dev.stderr


# ------------------------------------------------------------------------------------------ through the C ABI

def with_options(eng, opts, fn):
    for o, v in opts.items():
        eng.set_option(o, v)
    try:
        return fn()
    finally:
        for o in opts:
            eng.set_option(o, None)


def check_table(eng, t, n, k=21, kspace=KSPACE21, filters=FILTERS, routes=ROUTES):
    """labels, clusters and edges of every filter on every route against the model over mg_compare_tri_results_host's records;
    -> {filter: (labels, edges)}"""
    out = {}
    for fname, (max_d, max_p) in filters.items():
        rec = eng.compare_tri_results(t, k, kspace, max_d, max_p, capacity=1 << 22)
        want = np.array(cm.labels_fast(n, rec["row"], rec["col"]), dtype=np.uint32)
        for route, opts in routes.items():
            lab, nc, ne = with_options(eng, opts, lambda: eng.cluster_tri_host(t, k, kspace, max_d, max_p))
            assert ne == len(rec), (fname, route, ne, len(rec))
            assert np.array_equal(lab, want), (fname, route, int((lab != want).sum()))
            assert nc == int((want == np.arange(n)).sum()), (fname, route)
        out[fname] = (want, len(rec))
    return out


@pytest.mark.parametrize("n", [96, 4096, 20000])
def test_clustered_tables_every_filter_every_route(eng, n):
    table, nh, lengths = synth.clustered_sketches(n, 1000, clusters=max(3, n // 100), seed=3)
    t = eng.table_upload(table, nh, lengths)
    res = check_table(eng, t, n)
    lab, ne = res["d"]
    assert 0 < ne < n * (n - 1) // 2 and 1 < len(set(lab.tolist())) < n     # the filter bites, and something is joined
    t.free()


def test_one_species_chains_everywhere(eng):
    n = 4096
    table, nh, lengths = synth.species_sketches(n, 1000, seed=1)
    t = eng.table_upload(table, nh, lengths)
    res = check_table(eng, t, n)
    # -d 0.05 leaves a graph that is no union of cliques: some cluster has members that are not neighbours
    rec = eng.compare_tri_results(t, 21, KSPACE21, 0.05, -1.0, capacity=1 << 22)
    lab, ne = res["d"]
    sizes = np.bincount(lab, minlength=n).astype(np.int64)
    assert ne == len(rec) and ne < int((sizes * (sizes - 1) // 2).sum())
    # tighter thresholds: hundreds and thousands of clusters, still chains
    res = check_table(eng, t, n, filters={"d.03": (0.03, -1.0), "d.02": (0.02, -1.0)})
    for lab, ne in res.values():
        sizes = np.bincount(lab, minlength=n).astype(np.int64)
        assert 1 < len(set(lab.tolist())) < n and 0 < ne < int((sizes * (sizes - 1) // 2).sum())
    t.free()


def test_identical_rows_and_rows_without_edges(eng):
    rng = np.random.default_rng(9)
    n, s = 700, 256
    one = np.sort(rng.integers(0, 1 << 54, s, dtype=np.uint64))
    same = np.tile(one, (n, 1))
    t = eng.table_upload(same, np.full(n, s, dtype=np.uint32), np.full(n, 2_000_000, dtype=np.uint64))
    res = check_table(eng, t, n)
    assert res["d"][1] == n * (n - 1) // 2 and not res["d"][0].any()       # one clique, every label 0
    t.free()
    apart = np.sort(rng.integers(0, 1 << 54, (n, s), dtype=np.uint64), axis=1)
    t = eng.table_upload(apart, np.full(n, s, dtype=np.uint32), np.full(n, 2_000_000, dtype=np.uint64))
    res = check_table(eng, t, n)
    assert res["d"][1] == 0 and np.array_equal(res["d"][0], np.arange(n, dtype=np.uint32))
    t.free()


def test_block_boundaries_on_the_matrix_route(eng):
    """MASHGPU_CLUSTER_BLOCK_PAIRS cuts the matrix route into row blocks of that many pairs (a block always takes its first
    row): blocks of one row, of a few rows, and one block -- the parent array carries the clusters from block to block, and a
    cluster whose members lie in different blocks closes across the boundary"""
    n = 1200
    table, nh, lengths = synth.clustered_sketches(n, 1000, clusters=7, seed=5)
    perm = np.random.default_rng(2).permutation(n)                  # clusters interleave: every cluster spans every block
    table, nh, lengths = table[perm], nh[perm], lengths[perm]
    t = eng.table_upload(table, nh, lengths)
    routes = {f"blocks of {b} pairs": {"MASHGPU_RESULTS_MATRIX": "1", "MASHGPU_CLUSTER_BLOCK_PAIRS": str(b)} for b in (1, 4097, 100000, 1 << 30)}
    res = check_table(eng, t, n, filters={f: FILTERS[f] for f in ("d", "both")}, routes=routes)
    assert len(set(res["d"][0].tolist())) == 7
    t.free()


def test_against_the_oracle_own_distances_and_p_values(eng, oracle):
    """300 rows in five clusters (cliques) and 300 rows of one species (chains): the edges are the oracle's"""
    n = 300
    rows = np.concatenate([np.full(i, i) for i in range(n)])
    cols = np.concatenate([np.arange(i) for i in range(n)])
    for table, nh, lengths in (synth.clustered_sketches(n, 1000, clusters=5, seed=11), synth.species_sketches(n, 1000, seed=2)):
        lengths = np.asarray(lengths, dtype=np.uint64)
        _, _, dist, pval = oracle.triangle(table, nh, lengths, 0, n, 21, KSPACE21, stats=True)
        t = eng.table_upload(table, nh, lengths)
        for max_d, max_p in ((0.05, -1.0), (0.03, 1e-10), (-1.0, 1e-100), (0.02, 0.5)):
            keep = np.ones(len(dist), dtype=bool)
            if 0 <= max_d < 1:
                keep &= dist <= max_d                               # CommandDistance.cpp:409-412
            if 0 <= max_p < 1:
                keep &= pval <= max_p                               # :419-422
            want = np.array(cm.labels(n, rows[keep], cols[keep]), dtype=np.uint32)
            for route, opts in ROUTES.items():
                lab, nc, ne = with_options(eng, opts, lambda: eng.cluster_tri_host(t, 21, KSPACE21, max_d, max_p))
                assert ne == int(keep.sum()) and np.array_equal(lab, want) and nc == len(set(want.tolist())), (max_d, max_p, route)
        t.free()


# ------------------------------------------------------------------------------------------ calling conventions

def test_dev_form_and_repeated_calls(eng):
    import torch
    n = 4096
    table, nh, lengths = synth.species_sketches(n, 1000, seed=4)
    t = eng.table_upload(table, nh, lengths)
    for route, opts in ROUTES.items():
        first = with_options(eng, opts, lambda: eng.cluster_tri_host(t, 21, KSPACE21, 0.03, -1.0))
        for _ in range(2):
            again = with_options(eng, opts, lambda: eng.cluster_tri_host(t, 21, KSPACE21, 0.03, -1.0))
            assert np.array_equal(again[0], first[0]) and again[1:] == first[1:], route
        d_lab = torch.full((n + 1,), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
        nc, ne = with_options(eng, opts, lambda: eng.cluster_tri_dev(t, 21, KSPACE21, d_lab.data_ptr(), 0.03, -1.0))
        torch.cuda.synchronize()
        got = d_lab.cpu().numpy().view(np.uint32)
        assert got[n] == 0x7FFFFFFF and np.array_equal(got[:n], first[0]) and (nc, ne) == first[1:], route
    t.free()


def test_tables_of_no_and_one_row(eng):
    one = np.sort(np.random.default_rng(1).integers(0, 1 << 54, (1, 64), dtype=np.uint64), axis=1)
    t = eng.table_upload(one, np.full(1, 64, dtype=np.uint32), np.full(1, 1000, dtype=np.uint64))
    lab, nc, ne = eng.cluster_tri_host(t, 21, KSPACE21, 0.05, -1.0)
    assert list(lab) == [0] and (nc, ne) == (1, 0)
    t.free()
    t = eng.table_upload(np.zeros((0, 64), dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint64))
    lab, nc, ne = eng.cluster_tri_host(t, 21, KSPACE21, 0.05, -1.0)
    assert len(lab) == 0 and (nc, ne) == (0, 0)
    t.free()


def test_error_returns(eng):
    table, nh, lengths = synth.clustered_sketches(96, 1000, clusters=3, seed=1)
    t = eng.table_upload(table, nh, lengths)
    lab = np.zeros(96, dtype=np.uint32)
    nc, ne = C.c_uint64(0), C.c_uint64(0)

    def call(fn, max_d, max_p, k=21, table=t):
        return fn(eng.ctx, table.handle, k, KSPACE21, max_d, max_p, lab.ctypes.data, C.byref(nc), C.byref(ne))

    for fn in (eng.lib.mg_cluster_tri_host, eng.lib.mg_cluster_tri_dev):
        for max_d, max_p in ((-1.0, -1.0), (1.0, 1.0), (1.0, -1.0), (2.0, 1.5)):
            assert call(fn, max_d, max_p) == MG_ERR_INVALID
            assert b"both filters are off" in eng.lib.mg_last_error(eng.ctx)
    # everything else: as mg_compare_tri_results_host on the same arguments
    res = np.zeros(1 << 16, dtype=abi.RESULT_DTYPE)
    cnt = C.c_uint64(0)

    def results(max_d, max_p, k=21, table=t):
        return eng.lib.mg_compare_tri_results_host(eng.ctx, table.handle, 0, table.rows, k, KSPACE21, max_d, max_p, res.ctypes.data, len(res), C.byref(cnt))

    assert call(eng.lib.mg_cluster_tri_host, 0.05, -1.0, k=0) == results(0.05, -1.0, k=0) == MG_ERR_INVALID
    bare = eng.table_upload(table, nh, None)                        # a table without lengths, the p-value filter on
    for max_d, max_p in ((-1.0, 1e-10), (0.05, 1e-10)):
        want_rc = results(max_d, max_p, table=bare)
        want_edges = int(cnt.value)
        assert call(eng.lib.mg_cluster_tri_host, max_d, max_p, table=bare) == want_rc
        if want_rc == abi.MG_OK:
            assert int(ne.value) == want_edges
    assert call(eng.lib.mg_cluster_tri_host, 0.05, -1.0) == abi.MG_OK and int(nc.value) == 3      # the context still works
    bare.free()
    t.free()
