"""`mash triangle -H` / `mash dist -H` and mg_compare_tri_spectrum_host / mg_compare_rect_spectrum_host on the device.

1. Through the command: for every recording of tests/golden/knn (triangle; -d 0.08; -v 1e-10), topk (dist, the same three) and
   cluster (d1, d2, d3, v, dv) -- stdout of the REFERENCE CLI -- `-H` prints, byte for byte, what tests/spectrum_model.py makes of the
   recording: on the lists route, with the matrix forced, with the matrix in blocks of 100 pairs, with MASH_AMD_BLOCK_PAIRS=100 and
   on the host route (MASH_AMD_HOST_FINISH=1).
2. Filters off against the dense call (mg_compare_tri_host / mg_compare_rect_host, pinned to the oracle by tests/test_tri_gpu.py and
   tests/test_rect_gpu.py) plus np.unique: 300 rows of clades at s = 1000; the same with a fifth of the rows short, and with four rows
   empty besides; 40 rows at s = 20 000; rect with tables of s = 1000 and s = 500, and of s = 256 and s = 128 on the lists route (the
   rect suite's clean case); row and query ranges.  Every route gives the same
   bins and the stats name the route; on the arithmetic route a listed pair with numer 0 occurs.
3. Filters on against mg_compare_*_results_host plus np.unique: -d, -v and both, lists and matrix blocks; one species of 1 200 rows.
4. Hot bins: 300 identical rows (44 850 pairs in s/s) and 300 unrelated rows on the matrix route (all in 0/s), combining and plain.
5. Regrow: MASHGPU_SPECTRUM_SLOTS=4 on the short-sketch table gives the same bins with regrows > 0.
6. Calling conventions: capacity too small, the count-only call, repeated calls, 0- and 1-row tables, a p-value filter without
   lengths, null arguments.
Here, and only here, workgroups race on one bin: the emulator (tests/test_spectrum_emu.py) runs them one after another.  Every
command runs under its own timeout and every test under an alarm that ends the process; a non-zero exit ends the test."""
import ctypes as C
import json
import os
import signal
import subprocess

import numpy as np
import pytest

from mash_amd import abi
from tests import helpers
from tests import spectrum_model as sm
from workloads import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASH = os.path.join(ROOT, "mash_amd", "bin", "mash")
GOLD = os.path.join(ROOT, "tests", "golden")
KSPACE21 = 4.0 ** 21
MG_ERR_INVALID, MG_ERR_NOMEM = -1, -4              # include/mashgpu.h
PAD = np.uint64(0xFFFFFFFFFFFFFFFF)
KNOBS = ("MASH_AMD_HOST_FINISH", "MASH_AMD_BLOCK_PAIRS", "MASHGPU_RESULTS_MATRIX", "MASHGPU_SPECTRUM_BLOCK_PAIRS", "MASHGPU_SPECTRUM_PLAIN",
         "MASHGPU_SPECTRUM_SLOTS", "MASHGPU_COMPARE_KERNEL")


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

CLI_ROUTES = {"lists": {}, "lists, the index engine forced": {"MASHGPU_COMPARE_KERNEL": "sparse"}, "matrix": {"MASHGPU_RESULTS_MATRIX": "1"},
              "matrix in blocks of 100 pairs": {"MASHGPU_RESULTS_MATRIX": "1", "MASHGPU_SPECTRUM_BLOCK_PAIRS": "100"},
              "command blocks of 100 pairs": {"MASH_AMD_BLOCK_PAIRS": "100"},
              "host": {"MASH_AMD_HOST_FINISH": "1"}}


def mash(args, cwd, extra_env):
    env = dict(os.environ)
    for k in KNOBS:
        env.pop(k, None)
    env.update(extra_env)
    r = subprocess.run([MASH, *args], cwd=cwd, capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def recorded_commands():
    """(name, the reference's command without -E plus -H, working directory, recorded stdout) of every recording"""
    out = []
    knn = json.load(open(os.path.join(GOLD, "knn", "cases.json")))
    for c in knn["cases"]:
        args = [a for a in c["cmd"] if a != "-E"]
        out.append(("knn/" + c["name"], [*args, "-H", *knn["inputs"]], os.path.join(GOLD, knn["input_dir"]), os.path.join(GOLD, "knn", c["name"] + ".out")))
    topk = json.load(open(os.path.join(GOLD, "topk", "cases.json")))
    for c in topk["cases"]:
        out.append(("topk/" + c["name"], [*c["cmd"], "-H", *topk["inputs"]], os.path.join(GOLD, "topk"), os.path.join(GOLD, "topk", c["name"] + ".out")))
    cl = json.load(open(os.path.join(GOLD, "cluster", "cases.json")))
    for c in cl["cases"]:
        out.append(("cluster/" + c["name"], ["triangle", *cl["sketch"], *c["options"], "-H", cl["input"]], os.path.join(GOLD, "cluster"),
                    os.path.join(GOLD, "cluster", c["name"] + ".out")))
    return out


RECORDED = recorded_commands()


@pytest.mark.parametrize("name,args,cwd,recording", RECORDED, ids=[r[0] for r in RECORDED])
def test_command_on_the_recordings_every_route(name, args, cwd, recording):
    want = sm.spectrum_stdout(open(recording).read())
    assert want.count("\n") >= 2
    seen = set()
    for route, env in CLI_ROUTES.items():
        r = mash(args, cwd, env)
        assert r.stdout == want, (name, route, r.stdout[:400], want[:400])
        seen.add(r.stdout)
    assert len(seen) == 1


# ------------------------------------------------------------------------------------------ through the C ABI

def with_options(eng, opts, fn):
    for o, v in opts.items():
        eng.set_option(o, v)
    try:
        return fn()
    finally:
        for o in opts:
            eng.set_option(o, None)


LISTS = {"MASHGPU_COMPARE_KERNEL": "sparse"}              # (jobs this small are left to the tile engine unless the index engine is forced)
MATRIX = {"MASHGPU_RESULTS_MATRIX": "1"}
MATRIX_BLOCKS = {"MASHGPU_RESULTS_MATRIX": "1", "MASHGPU_SPECTRUM_BLOCK_PAIRS": "4097"}


def as_tuples(bins):
    return [(int(x["numer"]), int(x["denom"]), int(x["count"])) for x in bins]


def want_of(numer, denom):
    n, d, c = sm.spectrum_of_counts(numer, denom)
    return list(zip((int(x) for x in n), (int(x) for x in d), (int(x) for x in c)))


def clean_table():
    """300 rows of s = 1000 in six interleaved synthetic clades (no empty, short or copied row: the list engine takes the table); the
    last row shares one hash with row 5 and its relatives -- row 5's largest, which lies behind the 1000 smallest values of their
    union: listed pairs with numer 0"""
    rng = np.random.default_rng(20261021)
    table, nhash, _ = synth.clustered_sketches(300, 1000, clusters=6, seed=31)
    table = table.copy()
    n, s = table.shape
    assert n == 300 and (nhash == s).all()
    table[n - 1] = np.concatenate([np.arange(1, s, dtype=np.uint64), table[5, s - 1:]])
    lengths = rng.integers(10 ** 5, 10 ** 7, n).astype(np.uint64)
    return table, nhash, lengths


def short_table(empty):
    """clean_table with a fifth of its rows cut to 1 .. 999 hashes; empty: four rows without any"""
    table, nhash, lengths = clean_table()
    rng = np.random.default_rng(5)
    nhash = nhash.copy()
    for i in range(2, len(nhash) - 1, 5):
        nhash[i] = rng.integers(1, 1000)
    nhash[7], nhash[12] = 1, 999
    if empty:
        nhash[[3, 150, 151, 290]] = 0
    return helpers._pad_rows(table, nhash), nhash, lengths


@pytest.fixture(scope="module")
def tables(eng):
    """every table of the suite with its dense triangle (default engines), computed once"""
    out = {}
    big = helpers.clade_table(np.random.default_rng(8), (17, 17), 20000)
    made = {"clean": clean_table(), "short": short_table(False), "ragged": short_table(True),
            "s20000": (big[0], big[1], np.full(len(big[1]), 2_000_000, dtype=np.uint64))}
    for name, (table, nhash, lengths) in made.items():
        t = eng.table_upload(table, nhash, lengths)
        out[name] = {"t": t, "table": table, "nhash": nhash, "lengths": lengths, "n": len(nhash), "s": table.shape[1], "dense": eng.compare_tri_host(t)}
    yield out
    for v in out.values():
        v["t"].free()


def spectrum_tri(eng, c, opts, rb=0, re=None, max_d=-1.0, max_p=-1.0):
    got = with_options(eng, opts, lambda: eng.tri_spectrum(c["t"], 21, KSPACE21, max_d, max_p, rb, re))
    return as_tuples(got), eng.spectrum_stats()


def test_the_listed_pair_with_numer_zero_is_there(tables):
    """the choice of clean_table's last row, checked on the CPU: it shares a hash with row 5 and the dense call counts nothing"""
    c = tables["clean"]
    n, s = c["n"], c["s"]
    shares = helpers.shares_a_hash(c["table"], c["nhash"], c["table"][n - 1:], c["nhash"][n - 1:], s)[0]
    partners = np.nonzero(shares[:n - 1])[0]
    assert 5 in partners
    for j in partners:
        pair = c["dense"][helpers.tri_base(n - 1) + int(j)]
        assert (int(pair["numer"]), int(pair["denom"])) == (0, s)


@pytest.mark.parametrize("name", ["clean", "short", "ragged", "s20000"])
def test_filters_off_against_the_dense_call(eng, tables, name):
    c = tables[name]
    want = want_of(c["dense"]["numer"], c["dense"]["denom"])
    assert sum(x[2] for x in want) == c["n"] * (c["n"] - 1) // 2 and len(want) > 20
    if name in ("short", "ragged"):
        assert any(n == 0 and 0 < d < c["s"] for n, d, _ in want)                   # {0, D < s} occurs
    if name == "ragged":
        assert (0, 0, 6) in want and want[0] == (0, 0, 6)                            # four empty rows: six pairs of 0/0, ahead of s/s
    routes = {"default": ({}, 3), "matrix": (MATRIX, 3), "matrix in blocks": (MATRIX_BLOCKS, 3)}
    if name in ("clean", "short"):
        routes["lists"] = (LISTS, 2)
    seen = set()
    for route, (opts, number) in routes.items():
        got, stats = spectrum_tri(eng, c, opts)
        print(f"{name}, {route}: {stats}, {len(got)} bins")
        assert got == want, (name, route)
        assert stats["route"] == number and stats["regrows"] == 0, (name, route, stats)
        assert stats["other_keys"] == sum(1 for _, d, _ in want if d != c["s"]), (name, route, stats)
        if number == 2:
            assert stats["listed"] > 0 and (name != "clean" or stats["listed_zero"] >= 1), stats
        seen.add(tuple(got))
    assert len(seen) == 1


def test_row_ranges(eng, tables):
    c = tables["short"]
    n = c["n"]
    rng = np.random.default_rng(11)
    ranges = [(0, 1), (0, 2), (0, n), (1, n), (n - 1, n), (n, n), (n, n + 5), (250, 10 ** 9), (17, 17), (20, 10)]
    ranges += [tuple(sorted(int(x) for x in rng.integers(0, n + 1, 2))) for _ in range(4)]
    for rb, re in ranges:
        re_c = min(re, n)
        if rb >= re_c:
            want = []
        else:
            flat = helpers.tri_slice(c["dense"], rb, re_c)
            want = want_of(flat["numer"], flat["denom"]) if len(flat) else []
        for route, opts in (("lists", LISTS), ("matrix in blocks", MATRIX_BLOCKS)):
            got, stats = spectrum_tri(eng, c, opts, rb, re)
            assert got == want, (rb, re, route)
            assert stats["route"] == (0 if not want else 2 if route == "lists" else 3), (rb, re, route, stats)


@pytest.fixture(scope="module")
def rect(eng, tables):
    """references: the table with short rows (s = 1000); queries at s = 500: the first 500 hashes of every third reference and 20
    strangers -- `full` as they are (the index engine takes no query table with a short row), `short` with every ninth cut to
    1 .. 499 hashes: against a short reference its rule denominator is below 500"""
    c = tables["short"]
    rng = np.random.default_rng(13)
    rows = [c["table"][i, :500] for i in range(0, c["n"], 3)]
    rows += [np.unique(rng.integers(1, 1 << 60, 520).astype(np.uint64))[:500] for _ in range(20)]
    qt = np.stack(rows)
    qn = np.full(len(rows), 500, dtype=np.uint32)
    ql = rng.integers(10 ** 5, 10 ** 7, len(qn)).astype(np.uint64)
    qs = qn.copy()
    qs[4::9] = rng.integers(1, 500, len(qs[4::9]))
    full, short = eng.table_upload(qt, qn, ql), eng.table_upload(helpers._pad_rows(qt, qs), qs, ql)
    yield {"ref": c["t"], "nq": len(qn), "full": {"qry": full, "dense": eng.compare_rect_host(c["t"], full)},
           "short": {"qry": short, "dense": eng.compare_rect_host(c["t"], short)}}
    full.free()
    short.free()


@pytest.mark.parametrize("queries", ["full", "short"])
def test_rect_of_two_sketch_sizes(eng, rect, queries):
    nq, qry, dense = rect["nq"], rect[queries]["qry"], rect[queries]["dense"]
    routes = [("default", {}, (3,)), ("matrix in blocks", MATRIX_BLOCKS, (3,))]
    for qb, qe in ((0, nq), (0, 1), (5, 60), (nq - 1, nq + 3), (nq, nq), (40, 30)):
        block = dense[qb:min(qe, nq)] if qb < min(qe, nq) else dense[:0]
        want = want_of(block["numer"], block["denom"]) if block.size else []
        if (qb, qe) == (0, nq):
            assert all(d <= 500 for _, d, _ in want) and sum(x[2] for x in want) == nq * 300
            assert any(d < 500 for _, d, _ in want) == (queries == "short")
        for route, opts, numbers in routes:
            got = as_tuples(with_options(eng, opts, lambda: eng.rect_spectrum(rect["ref"], qry, 21, KSPACE21, -1.0, -1.0, qb, qe)))
            stats = eng.spectrum_stats()
            print(f"rect, {queries} queries [{qb}, {qe}), {route}: {stats}")
            assert got == want, (queries, qb, qe, route)
            assert stats["route"] in (numbers if want else (0,)), (queries, qb, qe, route, stats)


def test_rect_on_the_lists_route(eng):
    """the rect suite's clean case cut to s = 256 (references) and s = 128 (queries) -- 1 200 references the index engine takes, 87
    queries with copies, relatives, strangers, a short and an empty one: the lists with the rule against the dense call"""
    c = helpers.rect_case_sized(helpers.rect_case_clean(), 256, 128)
    ref, qry = eng.table_upload(c["rt"], c["rn"], c["rl"]), eng.table_upload(c["qt"], c["qn"], c["ql"])
    dense = eng.compare_rect_host(ref, qry)
    nq = len(c["qn"])
    for qb, qe in ((0, nq), (5, 60), (nq - 12, nq + 3), (0, 1)):
        block = dense[qb:min(qe, nq)]
        want = want_of(block["numer"], block["denom"])
        assert all(d <= 128 for _, d, _ in want) and sum(x[2] for x in want) == block.size
        for route, opts, numbers in (("lists", LISTS, (2,) if qe - qb > 8 else (2, 3)), ("default", {}, (3,)), ("matrix in blocks", MATRIX_BLOCKS, (3,))):
            got = as_tuples(with_options(eng, opts, lambda: eng.rect_spectrum(ref, qry, 21, KSPACE21, -1.0, -1.0, qb, qe)))
            stats = eng.spectrum_stats()
            print(f"rect clean 256 x 128, queries [{qb}, {qe}), {route}: {stats}")
            assert got == want, (qb, qe, route)
            assert stats["route"] in numbers, (qb, qe, route, stats)
        rec = eng.compare_rect_results(ref, qry, 21, KSPACE21, 0.1, -1.0, qb, qe)
        got = as_tuples(with_options(eng, LISTS, lambda: eng.rect_spectrum(ref, qry, 21, KSPACE21, 0.1, -1.0, qb, qe)))
        assert got == (want_of(rec["numer"], rec["denom"]) if len(rec) else []), (qb, qe)
    ref.free()
    qry.free()


# ------------------------------------------------------------------------------------------ 3. filters on

FILTERS = {"d": (0.05, -1.0), "v": (-1.0, 1e-30), "d and v": (0.2, 1e-10)}


@pytest.mark.parametrize("name", ["clean", "short", "ragged"])
def test_filters_on_against_the_results(eng, tables, name):
    c = tables[name]
    for what, (max_d, max_p) in FILTERS.items():
        rec = eng.compare_tri_results(c["t"], 21, KSPACE21, max_d, max_p)
        want = want_of(rec["numer"], rec["denom"])
        assert 0 < len(rec) < c["n"] * (c["n"] - 1) // 2
        routes = {"default": {}, "matrix in blocks": MATRIX_BLOCKS}
        if name != "ragged":
            routes["lists"] = LISTS
        for route, opts in routes.items():
            got, stats = spectrum_tri(eng, c, opts, max_d=max_d, max_p=max_p)
            assert got == want, (name, what, route)
            assert stats["route"] == 1 and sum(x[2] for x in got) == len(rec), (name, what, route, stats)
    rec = eng.compare_tri_results(c["t"], 21, KSPACE21, 0.05, -1.0, row_begin=100, row_end=220)
    got, _ = spectrum_tri(eng, c, MATRIX_BLOCKS, 100, 220, max_d=0.05)
    assert got == want_of(rec["numer"], rec["denom"])


def test_filters_on_rect(eng, rect):
    for what, (max_d, max_p) in FILTERS.items():
        rec = eng.compare_rect_results(rect["ref"], rect["full"]["qry"], 21, KSPACE21, max_d, max_p, 3, 90)
        want = want_of(rec["numer"], rec["denom"])
        assert len(rec) > 0
        for route, opts in (("default", {}), ("matrix in blocks", MATRIX_BLOCKS)):
            got = as_tuples(with_options(eng, opts, lambda: eng.rect_spectrum(rect["ref"], rect["full"]["qry"], 21, KSPACE21, max_d, max_p, 3, 90)))
            assert got == want and eng.spectrum_stats()["route"] == 1, (what, route)
        rec = eng.compare_rect_results(rect["ref"], rect["short"]["qry"], 21, KSPACE21, max_d, max_p)
        got = as_tuples(with_options(eng, MATRIX_BLOCKS, lambda: eng.rect_spectrum(rect["ref"], rect["short"]["qry"], 21, KSPACE21, max_d, max_p)))
        assert got == want_of(rec["numer"], rec["denom"]), what


def test_one_species(eng):
    """1 200 rows of one species: nearly every pair shares hashes; -d 0.05 and both filters, lists and matrix blocks, both variants"""
    n = 1200
    table, nh, lengths = synth.species_sketches(n, 1000, seed=7)
    t = eng.table_upload(table, nh, lengths)
    c = {"t": t}
    for max_d, max_p in ((0.05, -1.0), (0.08, 1e-200)):
        rec = eng.compare_tri_results(t, 21, KSPACE21, max_d, max_p, capacity=1 << 22)
        want = want_of(rec["numer"], rec["denom"])
        assert len(rec) > 64 and len(want) > 10
        seen = set()
        for opts in (LISTS, {}, MATRIX_BLOCKS, {**MATRIX_BLOCKS, "MASHGPU_SPECTRUM_PLAIN": "1"}, {**LISTS, "MASHGPU_SPECTRUM_PLAIN": "1"}):
            got, stats = spectrum_tri(eng, c, opts, max_d=max_d, max_p=max_p)
            assert got == want and stats["route"] == 1, (max_d, opts, stats)
            seen.add(tuple(got))
        assert len(seen) == 1
    t.free()


# ------------------------------------------------------------------------------------------ 4. hot bins

def test_hot_bins_both_variants(eng):
    rng = np.random.default_rng(3)
    row = np.unique(rng.integers(1, 1 << 60, 1100).astype(np.uint64))[:1000]
    same = np.tile(row, (300, 1))
    apart = np.sort(rng.integers(1, 1 << 60, (300, 1000)).astype(np.uint64), axis=1)
    nh, lengths = np.full(300, 1000, dtype=np.uint32), np.full(300, 1_000_000, dtype=np.uint64)
    for table, want in ((same, [(1000, 1000, 44850)]), (apart, [(0, 1000, 44850)])):
        t = eng.table_upload(table, nh, lengths)
        c = {"t": t}
        seen = set()
        for opts in ({}, MATRIX, MATRIX_BLOCKS, {"MASHGPU_SPECTRUM_PLAIN": "1"}, {**MATRIX_BLOCKS, "MASHGPU_SPECTRUM_PLAIN": "1"}):
            got, stats = spectrum_tri(eng, c, opts)
            assert got == want and stats["route"] == 3, (want, opts, got[:4], stats)
            seen.add(tuple(got))
        assert len(seen) == 1
        if table is same:                                    # with a filter every pair of the copies passes: the ballots are all ones
            for opts in ({}, {"MASHGPU_SPECTRUM_PLAIN": "1"}):
                got, stats = spectrum_tri(eng, c, opts, max_d=0.05)
                assert got == want and stats["route"] == 1, (opts, got[:4], stats)
        t.free()


# ------------------------------------------------------------------------------------------ 5. regrow

def test_regrow_from_four_slots(eng, tables):
    for name in ("short", "ragged"):
        c = tables[name]
        want = want_of(c["dense"]["numer"], c["dense"]["denom"])
        others = sum(1 for _, d, _ in want if d != c["s"])
        assert others > 64
        routes = [MATRIX, MATRIX_BLOCKS] + ([LISTS] if name == "short" else [])
        for opts in routes:
            got, stats = spectrum_tri(eng, c, {**opts, "MASHGPU_SPECTRUM_SLOTS": "4"})
            assert got == want, (name, opts)
            assert stats["regrows"] > 0 and stats["other_keys"] == others, (name, opts, stats)
        got, stats = spectrum_tri(eng, c, {"MASHGPU_SPECTRUM_SLOTS": "4"}, max_d=0.3)
        rec = eng.compare_tri_results(c["t"], 21, KSPACE21, 0.3, -1.0)
        assert got == want_of(rec["numer"], rec["denom"]) and stats["route"] == 1


# ------------------------------------------------------------------------------------------ 6. calling conventions

def test_capacity_count_only_and_repeated_calls(eng, tables):
    c = tables["short"]
    want = want_of(c["dense"]["numer"], c["dense"]["denom"])
    n = C.c_uint64(0)
    call = lambda out, cap: eng.lib.mg_compare_tri_spectrum_host(eng.ctx, c["t"].handle, 0, c["n"], 21, KSPACE21, -1.0, -1.0, out, cap, C.byref(n))
    assert call(None, 0) == MG_ERR_NOMEM and n.value == len(want)                  # the count alone
    buf = np.zeros(len(want), dtype=abi.SPECTRUM_DTYPE)
    buf["count"] = 77
    assert call(buf.ctypes.data, 3) == MG_ERR_NOMEM and n.value == len(want)
    assert b"capacity" in eng.lib.mg_last_error(eng.ctx)
    assert call(buf.ctypes.data, len(want)) == abi.MG_OK and n.value == len(want) and as_tuples(buf) == want
    for _ in range(3):
        got, _ = spectrum_tri(eng, c, {})
        assert got == want
    grown = eng.tri_spectrum(c["t"], 21, KSPACE21, capacity=2)                      # the wrapper asks again with the count it was told
    assert as_tuples(grown) == want


def test_tables_of_no_and_one_row(eng):
    one = np.sort(np.random.default_rng(1).integers(0, 1 << 54, (1, 64), dtype=np.uint64), axis=1)
    t = eng.table_upload(one, np.full(1, 64, dtype=np.uint32), np.full(1, 1000, dtype=np.uint64))
    assert len(eng.tri_spectrum(t, 21, KSPACE21)) == 0 and eng.spectrum_stats()["route"] == 0
    assert as_tuples(eng.rect_spectrum(t, t, 21, KSPACE21)) == [(64, 64, 1)]
    t.free()
    t = eng.table_upload(np.zeros((0, 64), dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint64))
    assert len(eng.tri_spectrum(t, 21, KSPACE21)) == 0 and len(eng.tri_spectrum(t, 21, KSPACE21, 0.05)) == 0
    assert len(eng.rect_spectrum(t, t, 21, KSPACE21)) == 0
    t.free()


def test_error_returns(eng, tables):
    c = tables["clean"]
    bare = eng.table_upload(c["table"], c["nhash"], None)
    buf = np.zeros(4096, dtype=abi.SPECTRUM_DTYPE)
    n = C.c_uint64(0)

    def tri(table=c["t"], k=21, max_d=-1.0, max_p=-1.0, out=buf.ctypes.data, cap=4096, n_ref=C.byref(n)):
        return eng.lib.mg_compare_tri_spectrum_host(eng.ctx, table.handle if table is not None else None, 0, 300, k, KSPACE21, max_d, max_p, out, cap, n_ref)

    def rect(ref=c["t"], qry=c["t"], max_p=-1.0, out=buf.ctypes.data, cap=4096, n_ref=C.byref(n)):
        return eng.lib.mg_compare_rect_spectrum_host(eng.ctx, ref.handle if ref is not None else None, qry.handle if qry is not None else None, 0, 10, 21,
                                                     KSPACE21, 0.05, max_p, out, cap, n_ref)

    assert tri(table=None) == MG_ERR_INVALID and tri(n_ref=None) == MG_ERR_INVALID and tri(out=None) == MG_ERR_INVALID
    assert b"NULL argument" in eng.lib.mg_last_error(eng.ctx)
    assert rect(ref=None) == MG_ERR_INVALID and rect(qry=None) == MG_ERR_INVALID and rect(n_ref=None) == MG_ERR_INVALID and rect(out=None) == MG_ERR_INVALID
    assert tri(k=0) == MG_ERR_INVALID
    assert tri(table=bare, max_p=1e-10) == MG_ERR_INVALID and b"no lengths" in eng.lib.mg_last_error(eng.ctx)
    assert tri(table=bare, max_d=0.05, max_p=0.5) == MG_ERR_INVALID
    assert rect(ref=bare, max_p=1e-10) == MG_ERR_INVALID and rect(qry=bare, max_p=1e-10) == MG_ERR_INVALID
    assert tri(table=bare) == abi.MG_OK and n.value > 20                             # without a p-value filter no length is read
    assert tri(table=bare, max_d=0.05, max_p=1.0) == abi.MG_OK
    assert eng.lib.mg_spectrum_stats(eng.ctx, None, None, None, None, None) == abi.MG_OK
    assert eng.lib.mg_spectrum_stats(None, None, None, None, None, None) == MG_ERR_INVALID
    assert tri() == abi.MG_OK and as_tuples(buf[:n.value]) == want_of(tables["clean"]["dense"]["numer"], tables["clean"]["dense"]["denom"])
    bare.free()
