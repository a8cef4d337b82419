"""`mash cluster -M` and mg_cluster_tri_medoid_host / mg_cluster_tri_medoid_dev on the device.

1. Through the command: for every recorded case of tests/golden/cluster (stdout of the REFERENCE CLI's `triangle -E`) the command
   prints, byte for byte, what tests/cluster_medoid_model.py makes of the recorded stdout -- on the candidate-list route, with the
   matrix route forced, with the matrix in row blocks of 100 pairs, and on the host route (MASH_AMD_HOST_FINISH=1); stderr is the same
   on every route; the same with -C; and `mash cluster` without -M still prints what tests/cluster_model.py makes of the recording.
2. A band table whose 300 scores have a closed form: one cluster, rows 3 .. 296 tie, row 3 is everybody's medoid.
3. Mixed denominators (21/63 beside 32/64 and 16/32, and 42/64 at a row that also has two 21/63), in both row orders, after the
   compared counts themselves have been checked to be that.
4. One species of 1 200 rows against the numpy model over mg_compare_tri_results_host's records: lists, matrix, matrix in blocks;
   the variant that combines a row's weights in the wave and the plain one give the same bits.
5. Calling conventions: the _dev form with guard words behind all three arrays, score = NULL, repeated calls, 0 and 1 rows, the
   error returns.
Here, and only here, workgroups race on score[], best[] and pick[]: the emulator (tests/test_cluster_medoid_emu.py) runs them one
after another.  Every command runs under its own timeout and every test under an alarm that ends the process; a non-zero exit
ends the test."""
import ctypes as C
import json
import os
import signal
import subprocess

import numpy as np
import pytest

from mash_amd import abi
from tests import cluster_medoid_model as mm
from tests import cluster_model as cm
from workloads import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASH = os.path.join(ROOT, "mash_amd", "bin", "mash")
GOLD = os.path.join(ROOT, "tests", "golden", "cluster")
KSPACE21 = 4.0 ** 21
MG_ERR_INVALID = -1             # include/mashgpu.h
PAD = np.uint64(0xFFFFFFFFFFFFFFFF)
ONE = 1 << 32


@pytest.fixture(autouse=True)
def time_limit():
    """a device call that hangs does not come back to the interpreter: the default action of SIGALRM ends the process"""
    old = signal.signal(signal.SIGALRM, signal.SIG_DFL)
    signal.alarm(240)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


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
              "host": {"MASH_AMD_HOST_FINISH": "1"}}


def mash(args, cwd, extra_env):
    env = dict(os.environ)
    for k in ("MASH_AMD_HOST_FINISH", "MASHGPU_RESULTS_MATRIX", "MASHGPU_CLUSTER_BLOCK_PAIRS", "MASHGPU_MEDOID_PLAIN"):
        env.pop(k, None)
    env.update(extra_env)
    r = subprocess.run([MASH, *args], cwd=cwd, capture_output=True, text=True, env=env, timeout=120)
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
    want = mm.medoid_stdout_of_triangle(texts[name], cases["names"])
    plain = cm.cluster_stdout_of_triangle(texts[name], cases["names"])
    assert [ln.rsplit("\t", 1)[0] for ln in want.splitlines()] == plain.splitlines()
    assert any(ln.split("\t")[3] != first for ln, first in zip(want.splitlines(), first_members(plain)))      # some medoid is not a first member
    args = [*cases["sketch"], *cluster_options(c["options"]), cases["input"]]
    errs = set()
    for route, env in CLI_ROUTES.items():
        r = mash(["cluster", "-M", *args], GOLD, env)
        assert r.stdout == want, (name, route)
        errs.add(r.stderr)
    assert len(errs) == 1
    assert mash(["cluster", *args], GOLD, {}).stdout == plain                     # without -M nothing has changed


def first_members(plain_stdout):
    """per line of `mash cluster` the ID of its cluster's first member"""
    first = {}
    for ln in plain_stdout.splitlines():
        number, _, name = ln.split("\t")
        first.setdefault(number, name)
    return [first[ln.split("\t")[0]] for ln in plain_stdout.splitlines()]


def test_command_with_comments():
    cases, texts = recorded()
    for name in ("d2", "dv"):
        opts = cluster_options([c["options"] for c in cases["cases"] if c["name"] == name][0])
        want_c = mm.medoid_stdout_of_triangle(texts[name], cases["names"], cases["comments"])
        for route in ("lists", "matrix in blocks of 100 pairs", "host"):
            r = mash(["cluster", "-M", "-C", *cases["sketch"], *opts, cases["input"]], GOLD, CLI_ROUTES[route])
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


ROUTES = {"lists": {}, "matrix": {"MASHGPU_RESULTS_MATRIX": "1"},
          "matrix in blocks of 4097 pairs": {"MASHGPU_RESULTS_MATRIX": "1", "MASHGPU_CLUSTER_BLOCK_PAIRS": "4097"}}
VARIANTS = {"combined in the wave": {}, "plain": {"MASHGPU_MEDOID_PLAIN": "1"}}


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
    """2. window_table(300, 1000, 100), threshold between 3 and 4 steps: one cluster; row i has the neighbours i +- 1, 2, 3 that
    exist, the pair k steps apart weighs floor((1000 - 100 k) * 2^32 / 1000); rows 3 .. 296 have all six and tie, row 3 wins"""
    n, s, step = 300, 1000, 100
    table, nh, lengths = window_table(n, s, step, seed=5)
    t = eng.table_upload(table, nh, lengths)
    d = [mash_distance(s - k * step, s) for k in range(6)]
    band_d = (d[3] + d[4]) / 2
    w = [0] + [(s - k * step) * ONE // s for k in (1, 2, 3)]
    want = [sum(w[k] for k in (1, 2, 3) if i - k >= 0) + sum(w[k] for k in (1, 2, 3) if i + k < n) for i in range(n)]
    assert want[3] == want[296] == 2 * sum((1000 - 100 * k) * ONE // 1000 for k in (1, 2, 3)) == max(want) and want[2] < want[3] > want[297]
    for route, opts in ROUTES.items():
        for variant, vopts in VARIANTS.items():
            label, medoid, score, nc, ne = with_options(eng, {**opts, **vopts}, lambda: eng.cluster_tri_medoid_host(t, 21, KSPACE21, band_d, -1.0))
            assert (nc, ne) == (1, 3 * n - 6), (route, variant)
            assert not label.any(), (route, variant)
            assert [int(x) for x in score] == want, (route, variant)
            assert (medoid == 3).all(), (route, variant, medoid[:8])
    t.free()


def mixed_rows():
    """s = 64.  From one pool: A has 64 hashes, M 32 of them, B 16 of those: M-A 32/64, M-B 16/32, A-B 16/64 (beyond -d 0.04).
    From a second pool of 84 + 22: X = q[0:42], Y = q[21:63], Z = q[42:84]: X-Y and Y-Z have 21 of a union of 63, X-Z nothing;
    W = Y and 22 hashes of its own, 64 in all: Y-W 42/64.  Row Y sums two weights of 21/63 and one of 42/64."""
    pool = np.unique(np.random.default_rng(9).integers(0, 1 << 54, 400, dtype=np.uint64))
    p, q = pool[:64], pool[64:64 + 84 + 22]
    return {"A": p, "M": p[::2], "B": p[::4], "X": q[0:42], "Y": q[21:63], "Z": q[42:84], "W": np.concatenate([q[21:63], q[84:106]])}


@pytest.mark.parametrize("order", ["AMBXYZW", "WZYXBMA", "YAXMWBZ"])
def test_mixed_denominators(eng, order):
    """3. the counts first, then scores and medoids exactly as the model has them"""
    s, rows = 64, mixed_rows()
    n = len(order)
    table = np.full((n, s), PAD, dtype=np.uint64)
    nh = np.zeros(n, dtype=np.uint32)
    for r, name in enumerate(order):
        table[r, :len(rows[name])] = np.sort(rows[name])
        nh[r] = len(rows[name])
    t = eng.table_upload(table, nh, np.full(n, 1_000_000, dtype=np.uint64))
    rec = eng.compare_tri_results(t, 21, KSPACE21, 0.04, -1.0)
    got = {frozenset((order[int(x["row"])], order[int(x["col"])])): (int(x["numer"]), int(x["denom"])) for x in rec}
    for pair, frac in {"AM": (32, 64), "MB": (16, 32), "XY": (21, 63), "YZ": (21, 63), "YW": (42, 64)}.items():
        assert got.get(frozenset(pair)) == frac, (pair, got)
    assert frozenset("AB") not in got and frozenset("XZ") not in got
    assert mm.weight(21, 63) * 3 != ONE and mm.weight(21, 63) == ONE // 3          # the weight that is no multiple of 2^-32
    lab, med, score = mm.medoid(n, rec["row"], rec["col"], rec["numer"], rec["denom"])
    y, m = order.index("Y"), order.index("M")
    assert score[y] == 2 * (ONE // 3) + 42 * ONE // 64 and score[m] == ONE and med[m] == m       # Y sums 63rds and 64ths; M beats A and B
    for route, opts in {"lists": {}, "matrix": {"MASHGPU_RESULTS_MATRIX": "1"}}.items():
        for variant, vopts in VARIANTS.items():
            label, medoid, sc, nc, ne = with_options(eng, {**opts, **vopts}, lambda: eng.cluster_tri_medoid_host(t, 21, KSPACE21, 0.04, -1.0))
            assert [int(x) for x in sc] == score, (order, route, variant)
            assert list(label) == lab and list(medoid) == med, (order, route, variant)
            assert (nc, ne) == (len(set(lab)), len(rec)), (order, route, variant)
    t.free()


@pytest.fixture(scope="module")
def species(eng):
    """one species of 1 200 rows with, per threshold, the model's answer over mg_compare_tri_results_host's records: computed once"""
    n = 1200
    table, nh, lengths = synth.species_sketches(n, 1000, seed=7)
    t = eng.table_upload(table, nh, lengths)
    want = {}
    for max_d in (0.05, 0.03):
        rec = eng.compare_tri_results(t, 21, KSPACE21, max_d, -1.0, capacity=1 << 22)
        lab, med, score = mm.medoid_fast(n, rec["row"], rec["col"], rec["numer"], rec["denom"])
        want[max_d] = (np.array(lab, dtype=np.uint32), np.array(med, dtype=np.uint32), np.array(score, dtype=np.uint64), len(rec))
    yield n, t, want
    t.free()


@pytest.mark.parametrize("max_d", [0.05, 0.03])
def test_one_species_every_route_and_variant(eng, species, max_d):
    """4. label, medoid, score, clusters and edges against the model; label, clusters and edges also against mg_cluster_tri_host"""
    n, t, want = species
    lab, med, score, ne_want = want[max_d]
    assert ne_want > 64 and (med != lab).any()                      # some cluster's medoid is not its first member
    label0, nc0, ne0 = eng.cluster_tri_host(t, 21, KSPACE21, max_d, -1.0)
    assert ne0 == ne_want and np.array_equal(label0, lab)
    seen = set()
    for route, opts in ROUTES.items():
        for variant, vopts in VARIANTS.items():
            label, medoid, sc, nc, ne = with_options(eng, {**opts, **vopts}, lambda: eng.cluster_tri_medoid_host(t, 21, KSPACE21, max_d, -1.0))
            print(f"species d {max_d} route {route}, {variant}: edges {ne} clusters {nc}, {len(mm.clusters_with_another_medoid(list(label), list(medoid)))} medoids that are not a first member")
            assert (nc, ne) == (nc0, ne0), (max_d, route, variant)
            assert np.array_equal(label, label0), (max_d, route, variant)
            assert np.array_equal(sc, score), (max_d, route, variant, int((sc != score).sum()))
            assert np.array_equal(medoid, med), (max_d, route, variant, int((medoid != med).sum()))
            seen.add((label.tobytes(), medoid.tobytes(), sc.tobytes()))
    assert len(seen) == 1                                           # every route, both variants: the same bits


# ------------------------------------------------------------------------------------------ 5. calling conventions

def test_dev_form_null_score_and_repeated_calls(eng, species):
    import torch
    n, t, want = species
    lab, med, score, ne_want = want[0.03]
    first = eng.cluster_tri_medoid_host(t, 21, KSPACE21, 0.03, -1.0)
    assert np.array_equal(first[0], lab) and np.array_equal(first[1], med) and np.array_equal(first[2], score) and first[4] == ne_want
    for with_score in (True, False, True):
        d_label = torch.full((n + 1,), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
        d_medoid = torch.full((n + 1,), 0x7FFFFFFE, dtype=torch.int32, device="cuda")
        d_score = torch.full((n + 1,), 0x7FFFFFFFFFFFFFFD, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        nc, ne = eng.cluster_tri_medoid_dev(t, 21, KSPACE21, d_label.data_ptr(), d_medoid.data_ptr(), d_score.data_ptr() if with_score else None, 0.03, -1.0)
        torch.cuda.synchronize()
        got_l, got_m, got_s = d_label.cpu().numpy().view(np.uint32), d_medoid.cpu().numpy().view(np.uint32), d_score.cpu().numpy().view(np.uint64)
        assert got_l[n] == 0x7FFFFFFF and got_m[n] == 0x7FFFFFFE and got_s[n] == 0x7FFFFFFFFFFFFFFD
        assert np.array_equal(got_l[:n], lab) and np.array_equal(got_m[:n], med) and (nc, ne) == first[3:]
        assert np.array_equal(got_s[:n], score) if with_score else (got_s[:n] == 0x7FFFFFFFFFFFFFFD).all()
    no_score = eng.cluster_tri_medoid_host(t, 21, KSPACE21, 0.03, -1.0, scores=False)
    assert no_score[2] is None and np.array_equal(no_score[0], lab) and np.array_equal(no_score[1], med) and no_score[3:] == first[3:]
    again = eng.cluster_tri_medoid_host(t, 21, KSPACE21, 0.03, -1.0)
    assert all(np.array_equal(again[k], first[k]) for k in range(3)) and again[3:] == first[3:]


def test_tables_of_no_and_one_row(eng):
    one = np.sort(np.random.default_rng(1).integers(0, 1 << 54, (1, 64), dtype=np.uint64), axis=1)
    t = eng.table_upload(one, np.full(1, 64, dtype=np.uint32), np.full(1, 1000, dtype=np.uint64))
    label, medoid, score, nc, ne = eng.cluster_tri_medoid_host(t, 21, KSPACE21, 0.05, -1.0)
    assert list(label) == [0] and list(medoid) == [0] and list(score) == [0] and (nc, ne) == (1, 0)
    t.free()
    t = eng.table_upload(np.zeros((0, 64), dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint64))
    label, medoid, score, nc, ne = eng.cluster_tri_medoid_host(t, 21, KSPACE21, 0.05, -1.0)
    assert len(label) == 0 and len(medoid) == 0 and len(score) == 0 and (nc, ne) == (0, 0)
    t.free()


def test_error_returns(eng):
    table, nh, lengths = synth.clustered_sketches(96, 1000, clusters=3, seed=1)
    t = eng.table_upload(table, nh, lengths)
    bare = eng.table_upload(table, nh, None)
    label, medoid = np.zeros(96, dtype=np.uint32), np.zeros(96, dtype=np.uint32)
    nc, ne = C.c_uint64(0), C.c_uint64(0)

    def call(fn, max_d, max_p, k=21, table=t, out=label.ctypes.data, out2=medoid.ctypes.data, nc_ref=C.byref(nc)):
        return fn(eng.ctx, table.handle if table is not None else None, k, KSPACE21, max_d, max_p, out, out2, None, nc_ref, C.byref(ne))

    for fn in (eng.lib.mg_cluster_tri_medoid_host, eng.lib.mg_cluster_tri_medoid_dev):
        for max_d, max_p in ((-1.0, -1.0), (1.0, 1.0), (1.0, -1.0), (2.0, 1.5)):
            assert call(fn, max_d, max_p) == MG_ERR_INVALID
            assert b"both filters are off" in eng.lib.mg_last_error(eng.ctx)
        assert call(fn, 0.05, -1.0, out=None) == MG_ERR_INVALID and b"NULL argument" in eng.lib.mg_last_error(eng.ctx)
        assert call(fn, 0.05, -1.0, out2=None) == MG_ERR_INVALID and b"NULL argument" in eng.lib.mg_last_error(eng.ctx)
        assert call(fn, 0.05, -1.0, table=None) == MG_ERR_INVALID
        assert call(fn, 0.05, -1.0, nc_ref=None) == MG_ERR_INVALID
        assert call(fn, 0.05, -1.0, table=bare) == MG_ERR_INVALID and b"no lengths" in eng.lib.mg_last_error(eng.ctx)
    assert call(eng.lib.mg_cluster_tri_medoid_host, 0.05, -1.0, k=0) == MG_ERR_INVALID
    assert call(eng.lib.mg_cluster_tri_medoid_host, 0.05, -1.0) == abi.MG_OK and int(nc.value) == 3      # the context still works
    bare.free()
    t.free()
