"""`mash cluster -A` and mg_cluster_extend_host / mg_cluster_extend_greedy_host on the device.

The judge is always the existing whole-table call (mg_cluster_tri_host, mg_cluster_tri_greedy_host) on `cat`, the rows of ref
followed by those of qry uploaded as ONE table, and the earlier result handed in is the existing call on ref: label / rep
equality, the number of clusters, and edges(ref) + new edges == edges(cat) -- on the candidate-list route, with the
inverted-index engine forced, on the matrix route, with the matrix in row blocks of 4 097 pairs over one parent array, and (greedy)
with an edge list that starts with room for 63 edges.  Tables: a path in index order split so that every new row joins two old
clusters, and so that two old clusters meet only through 100 new-new edges; 24 clades that all straddle the split; one species
(chains, many edges per new row); three chained extensions; the old representatives alone as ref; the calling conventions.
Through the command: tests/golden/cluster/family.fa.gz split into two FASTA files at L in {1, 17, 43}; `mash cluster -A` over
the earlier run's stdout prints, byte for byte, what the models make of the RECORDED reference `triangle -E` stdout for the whole
family, which is also what the run without -A prints -- plain and -R, device route and MASH_AMD_HOST_FINISH=1, with -C, from .msh
inputs, in blocks of 50 pairs, as a chain of two -A runs; and what is refused after sketching.
Here, and only here, workgroups race on the seeded arrays: the emulator (tests/test_cluster_extend_emu.py) runs them one after
another.  Every command runs under its own timeout."""
import ctypes as C
import gzip
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

ROUTES = {"default": {}, "sparse": {"MASHGPU_COMPARE_KERNEL": "sparse"}, "matrix": {"MASHGPU_RESULTS_MATRIX": "1"},
          "blocks": {"MASHGPU_RESULTS_MATRIX": "1", "MASHGPU_CLUSTER_BLOCK_PAIRS": "4097"}}
GREEDY_ROUTES = dict(ROUTES, **{"short list": {"MASHGPU_GREEDY_EDGE_CAP": "63"},
                                "blocks, short list": {"MASHGPU_RESULTS_MATRIX": "1", "MASHGPU_CLUSTER_BLOCK_PAIRS": "4097", "MASHGPU_GREEDY_EDGE_CAP": "63"}})


@pytest.fixture(scope="module")
def eng():
    import torch
    torch.cuda.init()          # (torch ships its own HIP runtime: it initialises first, tests/test_gpu_parity.py)
    e = abi.MashGpu(0)
    e.set_option("MASHGPU_COSTS_FIXED", "1")
    yield e
    e.close()


def with_options(eng, opts, fn):
    for o, v in opts.items():
        eng.set_option(o, v)
    try:
        return fn()
    finally:
        for o in opts:
            eng.set_option(o, None)


# ------------------------------------------------------------------------------------------ through the C ABI

class Split:
    """ref = the rows ref_idx of a table, qry = the rows qry_idx, cat = both as one table; the judge's results per filter"""

    def __init__(self, eng, table, nh, lengths, ref_idx, qry_idx):
        self.eng = eng
        order = np.concatenate([ref_idx, qry_idx]).astype(np.int64)
        self.n, self.m = len(ref_idx), len(qry_idx)
        self.parts = (table[order], nh[order], lengths[order])
        self.cat = eng.table_upload(*self.parts)
        self.ref = eng.table_upload(*(x[: self.n] for x in self.parts))
        self.qry = eng.table_upload(*(x[self.n:] for x in self.parts))

    def free(self):
        for t in (self.cat, self.ref, self.qry):
            t.free()

    def check(self, max_d, max_p, k=21, kspace=KSPACE21, routes=ROUTES, greedy_routes=GREEDY_ROUTES):
        """both modes on every route against the whole-table calls on cat; -> what the judge said"""
        eng, n, m = self.eng, self.n, self.m
        lab_cat, nc_cat, ne_cat = eng.cluster_tri_host(self.cat, k, kspace, max_d, max_p)
        lab_ref, nc_ref, ne_ref = eng.cluster_tri_host(self.ref, k, kspace, max_d, max_p)
        rep_cat, ncg_cat, neg_cat = eng.cluster_tri_greedy_host(self.cat, k, kspace, max_d, max_p)
        rep_ref, ncg_ref, neg_ref = eng.cluster_tri_greedy_host(self.ref, k, kspace, max_d, max_p)
        assert neg_cat == ne_cat and neg_ref == ne_ref and np.array_equal(rep_cat[:n], rep_ref)       # the old rows never change
        for route, opts in routes.items():
            lab, nc, ne = with_options(eng, opts, lambda: eng.cluster_extend_host(self.ref, self.qry, lab_ref, k, kspace, max_d, max_p))
            print(f"n {n} m {m} d {max_d} p {max_p} route {route}: single linkage: new edges {ne} of {ne_cat}, clusters {nc_ref} -> {nc}")
            assert np.array_equal(lab, lab_cat), (route, int((lab != lab_cat).sum()))
            assert nc == nc_cat and ne_ref + ne == ne_cat, (route, nc, nc_cat, ne_ref, ne, ne_cat)
        for route, opts in greedy_routes.items():
            rep, nc, ne = with_options(eng, opts, lambda: eng.cluster_extend_greedy_host(self.ref, self.qry, rep_ref, k, kspace, max_d, max_p))
            st = eng.cluster_greedy_stats()
            print(f"n {n} m {m} d {max_d} p {max_p} route {route}: greedy: new edges {ne} of {ne_cat}, representatives {ncg_ref} -> {nc}, {st}")
            assert np.array_equal(rep, rep_cat[n:]), (route, int((rep != rep_cat[n:]).sum()))
            assert nc == ncg_cat and ne_ref + ne == ne_cat, (route, nc, ncg_cat, ne_ref, ne, ne_cat)
            assert 1 <= st["rounds"] <= n + m and st["batches"] >= 1 and st["edge_capacity"] >= min(ne, 1)
            if "MASHGPU_GREEDY_EDGE_CAP" in opts and ne > int(opts["MASHGPU_GREEDY_EDGE_CAP"]):
                assert st["regrows"] >= 1, (route, st)
        return dict(lab_cat=lab_cat, nc_cat=nc_cat, ne_cat=ne_cat, nc_ref=nc_ref, ne_ref=ne_ref, rep_cat=rep_cat, rep_ref=rep_ref, ncg_cat=ncg_cat)


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


def test_path_every_new_row_joins_two_old_clusters(eng):
    n_all = 600
    table, nh, lengths = window_table(n_all, 1000, 100, seed=6)
    path_d = (mash_distance(900, 1000) + mash_distance(800, 1000)) / 2          # the only edges are (i, i + 1)
    i = np.arange(n_all)
    sp = Split(eng, table, nh, lengths, i[i % 3 != 1], i[i % 3 == 1])
    got = sp.check(path_d, -1.0)
    # ref alone: rows 3 k + 2 and 3 k + 3 are neighbours, row 0 has none: 1 + 199 pairs + row 599; every new row 3 k + 1 joins two of them
    assert got["nc_ref"] > 190 and got["nc_cat"] == 1 and got["ne_cat"] == n_all - 1
    sp.free()


def test_path_old_clusters_meet_through_new_rows_only(eng):
    n_all = 600
    table, nh, lengths = window_table(n_all, 1000, 100, seed=6)
    path_d = (mash_distance(900, 1000) + mash_distance(800, 1000)) / 2
    i = np.arange(n_all)
    sp = Split(eng, table, nh, lengths, np.concatenate([i[:300], i[400:]]), i[300:400])
    got = sp.check(path_d, -1.0)
    assert got["nc_ref"] == 2 and got["nc_cat"] == 1 and got["ne_cat"] - got["ne_ref"] == 101      # 99 new-new edges and the two ends
    sp.free()


def test_clades_that_straddle_the_split(eng):
    n_all, n = 2448, 1931
    table, nh, lengths = synth.clustered_sketches(n_all, 1000, clusters=24, seed=5)
    perm = np.random.default_rng(20261020).permutation(n_all)
    sp = Split(eng, table, nh, lengths, perm[:n], perm[n:])
    for max_d, max_p in ((0.05, -1.0), (0.05, 1e-10)):
        got = sp.check(max_d, max_p)
        assert 0 < got["ne_cat"] < n_all * (n_all - 1) // 2 and 0 < got["ne_ref"] < got["ne_cat"]      # the filter bites
        assert 1 < got["nc_cat"] < n_all
    sp.free()


def test_one_species_chains(eng):
    n_all, n = 1200, 777
    table, nh, lengths = synth.species_sketches(n_all, 1000, seed=1)
    i = np.arange(n_all)
    sp = Split(eng, table, nh, lengths, i[:n], i[n:])
    got = sp.check(0.03, -1.0)
    assert got["ne_cat"] > got["ne_ref"] > 0 and not np.array_equal(got["rep_cat"], got["lab_cat"])      # chains: greedy is finer
    assert np.array_equal(got["lab_cat"][got["rep_cat"]], got["lab_cat"])                               # ... and refines single linkage
    sp.free()


def test_three_chained_extensions_and_representatives_alone(eng):
    n_all = 1200
    table, nh, lengths = synth.species_sketches(n_all, 1000, seed=1)
    whole = eng.table_upload(table, nh, lengths)
    lab_all, nc_all, ne_all = eng.cluster_tri_host(whole, 21, KSPACE21, 0.03, -1.0)
    rep_all, ncg_all, _ = eng.cluster_tri_greedy_host(whole, 21, KSPACE21, 0.03, -1.0)
    whole.free()

    def part(a, b):
        return eng.table_upload(table[a:b], nh[a:b], lengths[a:b])

    first = part(0, 400)
    lab, _, edges = eng.cluster_tri_host(first, 21, KSPACE21, 0.03, -1.0)
    rep, _, _ = eng.cluster_tri_greedy_host(first, 21, KSPACE21, 0.03, -1.0)
    first.free()
    for a, b in ((400, 800), (800, 1200)):
        ref, qry = part(0, a), part(a, b)
        lab, nc, ne = eng.cluster_extend_host(ref, qry, lab, 21, KSPACE21, 0.03, -1.0)
        more, ncg, neg = eng.cluster_extend_greedy_host(ref, qry, rep, 21, KSPACE21, 0.03, -1.0)
        # the same step with the old representatives alone as ref
        keep = np.flatnonzero(rep == np.arange(a)).astype(np.int64)
        small = eng.table_upload(table[keep], nh[keep], lengths[keep])
        got, ncs, _ = eng.cluster_extend_greedy_host(small, qry, None, 21, KSPACE21, 0.03, -1.0)
        back = np.concatenate([keep, np.arange(a, b)]).astype(np.uint32)
        assert np.array_equal(back[got], more) and ncs == ncg and len(keep) < a
        rep = np.concatenate([rep, more])
        edges += ne
        assert neg == ne
        for t in (ref, qry, small):
            t.free()
    assert np.array_equal(lab, lab_all) and nc == nc_all and edges == ne_all
    assert np.array_equal(rep, rep_all) and ncg == ncg_all


# ------------------------------------------------------------------------------------------ calling conventions

def small_tables(eng, n, m, s=64, seed=2):
    table, nh, lengths = synth.clustered_sketches(n + m, s, clusters=3, seed=seed)
    return (table, nh, lengths), eng.table_upload(table[:n], nh[:n], lengths[:n]), eng.table_upload(table[n:], nh[n:], lengths[n:])


def test_no_new_rows_no_old_rows_one_row_each(eng):
    (table, nh, lengths), ref, none = small_tables(eng, 96, 0, s=1000, seed=1)
    lab_ref, nc_ref, _ = eng.cluster_tri_host(ref, 21, KSPACE21, 0.05, -1.0)
    rep_ref, ncg_ref, _ = eng.cluster_tri_greedy_host(ref, 21, KSPACE21, 0.05, -1.0)
    # m = 0: the input comes back
    lab, nc, ne = eng.cluster_extend_host(ref, none, lab_ref, 21, KSPACE21, 0.05, -1.0)
    assert np.array_equal(lab, lab_ref) and (nc, ne) == (nc_ref, 0)
    rep, nc, ne = eng.cluster_extend_greedy_host(ref, none, rep_ref, 21, KSPACE21, 0.05, -1.0)
    assert len(rep) == 0 and (nc, ne) == (ncg_ref, 0)
    rep, nc, ne = eng.cluster_extend_greedy_host(ref, none, None, 21, KSPACE21, 0.05, -1.0)
    assert len(rep) == 0 and (nc, ne) == (96, 0)
    # n = 0: the whole-table call on qry
    lab, nc, ne = eng.cluster_extend_host(none, ref, np.zeros(0, dtype=np.uint32), 21, KSPACE21, 0.05, -1.0)
    assert np.array_equal(lab, lab_ref) and nc == nc_ref and ne > 0
    for seed in (np.zeros(0, dtype=np.uint32), None):
        rep, nc, ne2 = eng.cluster_extend_greedy_host(none, ref, seed, 21, KSPACE21, 0.05, -1.0)
        assert np.array_equal(rep, rep_ref) and nc == ncg_ref and ne2 == ne
    # neither
    lab, nc, ne = eng.cluster_extend_host(none, none, np.zeros(0, dtype=np.uint32), 21, KSPACE21, 0.05, -1.0)
    assert len(lab) == 0 and (nc, ne) == (0, 0)
    rep, nc, ne = eng.cluster_extend_greedy_host(none, none, None, 21, KSPACE21, 0.05, -1.0)
    assert len(rep) == 0 and (nc, ne) == (0, 0)
    # one row each, under a threshold nearly every related pair passes and under one no pair of distinct rows passes
    one, two = eng.table_upload(table[:1], nh[:1], lengths[:1]), eng.table_upload(table[1:2], nh[1:2], lengths[1:2])
    both = eng.table_upload(table[:2], nh[:2], lengths[:2])
    for max_d in (0.9, 1e-6):
        want = eng.cluster_tri_host(both, 21, KSPACE21, max_d, -1.0)
        lab, nc, ne = eng.cluster_extend_host(one, two, [0], 21, KSPACE21, max_d, -1.0)
        assert np.array_equal(lab, want[0]) and (nc, ne) == want[1:]
        rep, ncg, neg = eng.cluster_extend_greedy_host(one, two, [0], 21, KSPACE21, max_d, -1.0)
        assert list(rep) == [want[0][1]] and (ncg, neg) == want[1:]
    for t in (ref, none, one, two, both):
        t.free()


def test_error_returns_and_repeated_calls(eng):
    (table, nh, lengths), ref, qry = small_tables(eng, 60, 36, s=1000, seed=1)
    other_s = eng.table_upload(table[:10, :64], np.full(10, 64, dtype=np.uint32), lengths[:10])
    lab_ref, _, _ = eng.cluster_tri_host(ref, 21, KSPACE21, 0.05, -1.0)
    assert len(set(lab_ref.tolist())) < 60                     # some row is not its own label
    out = np.zeros(96, dtype=np.uint32)
    nc, ne = C.c_uint64(0), C.c_uint64(0)

    def call(fn, seed, max_d=0.05, max_p=-1.0, k=21, r=ref, q=qry, o=out.ctypes.data):
        seed = None if seed is None else np.ascontiguousarray(seed, dtype=np.uint32)
        return fn(eng.ctx, r.handle, q.handle, None if seed is None else seed.ctypes.data, k, KSPACE21, max_d, max_p, o, C.byref(nc), C.byref(ne))

    def message():
        return eng.lib.mg_last_error(eng.ctx).decode()

    for fn, name in ((eng.lib.mg_cluster_extend_host, "ref_label"), (eng.lib.mg_cluster_extend_greedy_host, "ref_rep")):
        for max_d, max_p in ((-1.0, -1.0), (1.0, 1.0), (1.0, -1.0), (2.0, 1.5)):
            assert call(fn, lab_ref, max_d, max_p) == MG_ERR_INVALID and "both filters are off" in message()
        assert call(fn, lab_ref, q=other_s) == MG_ERR_INVALID and "sketch sizes differ" in message()
        assert call(fn, lab_ref[:10], r=other_s) == MG_ERR_INVALID and "sketch sizes differ" in message()
        assert call(fn, lab_ref, o=None) == MG_ERR_INVALID
        assert call(fn, lab_ref, k=0) == MG_ERR_INVALID
        bad = lab_ref.copy()
        bad[7] = 8                                             # larger than its row
        assert call(fn, bad) == MG_ERR_INVALID and f"{name}[7] = 8 is larger than its row" in message()
        member = int(np.flatnonzero(lab_ref != np.arange(60))[0])
        later = int(np.flatnonzero(np.arange(60) > member)[0])
        bad = lab_ref.copy()
        bad[later] = member                                    # a label that is not the first row of its cluster
        assert call(fn, bad) == MG_ERR_INVALID and f"{name}[{later}] = {member} is not the first row" in message()
    assert call(eng.lib.mg_cluster_extend_host, None) == MG_ERR_INVALID                  # NULL only where NULL means something
    # the context still works, and repeated calls give equal output
    first = eng.cluster_extend_host(ref, qry, lab_ref, 21, KSPACE21, 0.05, -1.0)
    again = eng.cluster_extend_host(ref, qry, lab_ref, 21, KSPACE21, 0.05, -1.0)
    assert np.array_equal(first[0], again[0]) and first[1:] == again[1:]
    rep_ref, _, _ = eng.cluster_tri_greedy_host(ref, 21, KSPACE21, 0.05, -1.0)
    first = eng.cluster_extend_greedy_host(ref, qry, rep_ref, 21, KSPACE21, 0.05, -1.0)
    again = eng.cluster_extend_greedy_host(ref, qry, rep_ref, 21, KSPACE21, 0.05, -1.0)
    assert np.array_equal(first[0], again[0]) and first[1:] == again[1:]
    for t in (ref, qry, other_s):
        t.free()


# ------------------------------------------------------------------------------------------ through the command

def mash(args, cwd, extra_env=None, ok=True):
    env = dict(os.environ)
    for k in ("MASH_AMD_HOST_FINISH", "MASH_AMD_BLOCK_PAIRS", "MASHGPU_RESULTS_MATRIX", "MASHGPU_CLUSTER_BLOCK_PAIRS", "MASHGPU_GREEDY_EDGE_CAP"):
        env.pop(k, None)
    env.update(extra_env or {})
    r = subprocess.run([MASH, *args], cwd=cwd, capture_output=True, text=True, env=env, timeout=300)
    assert (r.returncode == 0) == ok, r.stderr[-2000:]
    return r


HOST = {"MASH_AMD_HOST_FINISH": "1"}


def cluster_options(triangle_options):
    """triangle's -d defaults to 1, cluster's to 0.05: a recording without -d is matched by an explicit -d 1"""
    return list(triangle_options) if "-d" in triangle_options else ["-d", "1", *triangle_options]


@pytest.fixture(scope="module")
def family(tmp_path_factory):
    """the recorded cases; what the models make of the recorded `triangle -E` stdout, per case and mode; the family's records"""
    cases = json.load(open(os.path.join(GOLD, "cases.json")))
    texts = {c["name"]: open(os.path.join(GOLD, c["name"] + ".out")).read() for c in cases["cases"]}
    want = {}
    for name, text in texts.items():
        for greedy, model in ((False, cm.cluster_stdout_of_triangle), (True, gm.greedy_stdout_of_triangle)):
            want[name, greedy] = model(text, cases["names"])
            want[name, greedy, "-C"] = model(text, cases["names"], cases["comments"])
    records = [">" + r for r in gzip.open(os.path.join(GOLD, cases["input"]), "rt").read().split(">")[1:]]
    assert len(records) == len(cases["names"]) == 44
    return cases, want, records


def split_at(records, tmp_path, *cuts):
    """the records in FASTA files cut at `cuts`: a.fa, b.fa, ..."""
    names, at = [], [0, *cuts, len(records)]
    for k in range(len(at) - 1):
        names.append("abcdef"[k] + ".fa")
        (tmp_path / names[-1]).write_text("".join(records[at[k]: at[k + 1]]))
    return names


@pytest.mark.parametrize("L", [1, 17, 43])
def test_command_on_the_recorded_family_split_in_two(family, tmp_path, L):
    cases, want, records = family
    a, b = split_at(records, tmp_path, L)
    for c in cases["cases"]:
        opts = [*cases["sketch"], *cluster_options(c["options"])]
        for greedy in (False, True):
            mode = ["-R"] if greedy else []
            (tmp_path / "old").write_text(mash(["cluster", *mode, *opts, a], tmp_path).stdout)
            dev = mash(["cluster", "-A", "old", *mode, *opts, a, b], tmp_path)
            host = mash(["cluster", "-A", "old", *mode, *opts, a, b], tmp_path, HOST)
            assert dev.stdout == want[c["name"], greedy], (c["name"], greedy, "device route")
            assert host.stdout == want[c["name"], greedy], (c["name"], greedy, "host route")
            assert dev.stderr == host.stderr
            plain = mash(["cluster", *mode, *opts, a, b], tmp_path)
            assert plain.stdout == dev.stdout and plain.stderr == dev.stderr, (c["name"], greedy, "the run without -A")


def test_command_with_comments_msh_inputs_small_blocks_and_a_chain(family, tmp_path):
    cases, want, records = family
    a, b, c3 = split_at(records, tmp_path, 10, 30)
    for name in ("dv",):
        opts = [*cases["sketch"], *cluster_options([c["options"] for c in cases["cases"] if c["name"] == name][0])]
        for greedy in (False, True):
            mode = ["-R"] if greedy else []
            # a chain of two -A runs, the second over the first one's output
            (tmp_path / "old").write_text(mash(["cluster", *mode, *opts, a], tmp_path).stdout)
            (tmp_path / "older").write_text(mash(["cluster", "-A", "old", *mode, *opts, a, b], tmp_path).stdout)
            assert (tmp_path / "older").read_text() == mash(["cluster", *mode, *opts, a, b], tmp_path).stdout
            for env in ({}, HOST, {"MASH_AMD_BLOCK_PAIRS": "50"}, dict(HOST, MASH_AMD_BLOCK_PAIRS="50"),
                        {"MASHGPU_RESULTS_MATRIX": "1", "MASHGPU_CLUSTER_BLOCK_PAIRS": "100", "MASHGPU_GREEDY_EDGE_CAP": "7"}):
                assert mash(["cluster", "-A", "older", *mode, *opts, a, b, c3], tmp_path, env).stdout == want[name, greedy], (name, greedy, env)
            # -C: the IDs of the earlier output are the comments
            (tmp_path / "oldc").write_text(mash(["cluster", "-C", *mode, *opts, a, b], tmp_path).stdout)
            for env in ({}, HOST):
                assert mash(["cluster", "-C", "-A", "oldc", *mode, *opts, a, b, c3], tmp_path, env).stdout == want[name, greedy, "-C"], (name, greedy, env)
    # .msh inputs
    opts = cluster_options([c["options"] for c in cases["cases"] if c["name"] == "d2"][0])
    for f in (a, b, c3):
        mash(["sketch", *cases["sketch"], "-o", f[0], f], tmp_path)
    for greedy in (False, True):
        mode = ["-R"] if greedy else []
        (tmp_path / "oldm").write_text(mash(["cluster", *mode, *opts, "a.msh", "b.msh"], tmp_path).stdout)
        for env in ({}, HOST):
            assert mash(["cluster", "-A", "oldm", *mode, *opts, "a.msh", "b.msh", "c.msh"], tmp_path, env).stdout == want["d2", greedy], (greedy, env)


def error_line(r):
    """exit status 1, empty stdout and, behind the sketching's progress lines, ONE ERROR line: that line"""
    lines = r.stderr.splitlines()
    assert r.returncode == 1 and r.stdout == "" and [ln.startswith("ERROR: ") for ln in lines].count(True) == 1 and r.stderr.endswith("\n"), r.stderr
    assert lines[-1].startswith("ERROR: ") and all(ln.startswith("Sketching ") for ln in lines[:-1]), r.stderr
    return lines[-1]


def test_command_refusals_after_sketching(family, tmp_path):
    cases, want, records = family
    a, b = split_at(records, tmp_path, 17)
    opts = [*cases["sketch"], "-d", "0.1"]
    old = mash(["cluster", *opts, a], tmp_path).stdout
    lines = old.splitlines(True)
    # a name that is not the input's
    lines[4] = lines[4].replace("g04", "g40")
    (tmp_path / "renamed").write_text("".join(lines))
    for env in ({}, HOST):
        r = mash(["cluster", "-A", "renamed", *opts, a, b], tmp_path, env, ok=False)
        err = error_line(r)
        assert err.startswith("ERROR: Line 5 of renamed ") and '"g40"' in err and '"g04"' in err
    # the names are there, the comments are asked for
    (tmp_path / "old").write_text(old)
    r = mash(["cluster", "-C", "-A", "old", *opts, a, b], tmp_path, ok=False)
    err = error_line(r)
    assert err.startswith("ERROR: Line 1 of old ") and '"g00"' in err and "member 00 of clade 2" in err
    # the later inputs alone
    r = mash(["cluster", "-A", "old", *opts, b], tmp_path, ok=False)
    err = error_line(r)
    assert err.startswith("ERROR: Line 1 of old ") and '"g00"' in err and '"g17"' in err
    # more lines than inputs
    both = mash(["cluster", *opts, a, b], tmp_path).stdout
    (tmp_path / "all").write_text(both)
    r = mash(["cluster", "-A", "all", *opts, a], tmp_path, ok=False)
    assert error_line(r) == "ERROR: all has 44 lines, but there are only 17 input sequences."
    # every input was there already: the earlier output comes back
    for env in ({}, HOST):
        assert mash(["cluster", "-A", "all", *opts, a, b], tmp_path, env).stdout == both
