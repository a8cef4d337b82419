#!/usr/bin/env python3
"""What the finished rows of `mash screen` cost: mg_screen_results_host beside mg_screen_finish_sparse_host on the same
mixture, and the whole command beside another build of it (the parent commit with the same MASH_AMD_TIMING laps).

    python tools/screen_results_bench.py [--db 100000] [--reps 20] [--parent-mash path/to/parent/bin/mash] [--cli-runs 5]

Two databases of `--db` sketches (k = 21, s = 1000) of synthetic genomes of 1300 bases: `clusters100`, clusters of 100
relatives (the cluster size of the filler in tools/screen_bench.py), and `clades1000`, clades of 1000 relatives (members
at 0 - 4 % from their ancestor).  Mixtures are whole genomes of rows chosen so that the mixture touches about 0.1 %, 1 %
and 10 % of the rows (a genome touches its relatives too: the rows really touched are recorded).  Per cell, with and
without `winner`: 3 warm-ups, then `--reps` timed repetitions of results() (sizing call + fetch, what a caller pays) and
of finish_sparse(), HIP events around each and wall time ending in a synchronise; median, min and max.
With --parent-mash: the same database and mixture as .msh / FASTA files, both commands alternating, `--cli-runs` runs
each with MASH_AMD_TIMING=1, each run under its own time limit; the laps `screen`, `results` / `host tail` are recorded.
Writes profiles/screen_results_bench.json and prints it."""
import argparse, json, os, re, shutil, statistics, subprocess, sys, tempfile, time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from mash_amd.abi import MashGpu  # noqa: E402

K, S, L = 21, 1000, 1300
MASH = os.path.join(ROOT, "mash_amd", "bin", "mash")


def make_genomes(n, per, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    anc = torch.randint(0, 4, (n // per, L), dtype=torch.uint8, device="cuda", generator=g)
    codes = anc.repeat_interleave(per, 0)
    rate = torch.linspace(0.0, 0.04, per, device="cuda").repeat(n // per)
    mut = torch.rand((n, L), device="cuda", generator=g) < rate[:, None]
    codes = torch.where(mut, torch.randint(0, 4, (n, L), dtype=torch.uint8, device="cuda", generator=g), codes)
    return torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")[codes.long()].contiguous()


def mixture(bases, per, frac):
    """whole genomes of about frac * n rows, taken from as few clusters as hold them, each twice and its first half a third
    time (uneven depth), records separated by a newline"""
    n = bases.shape[0]
    want = max(1, round(frac * n))
    ncl = max(1, want // per)
    step = max(1, (n // per) // ncl)
    src = torch.cat([torch.arange(c * step * per, c * step * per + min(per, want // ncl), device="cuda") for c in range(ncl)])
    sep = torch.full((len(src), 1), 0x0A, dtype=torch.uint8, device="cuda")
    whole = torch.cat([bases[src], sep], 1).flatten()
    half = torch.cat([bases[src][:, : L // 2], sep], 1).flatten()
    return torch.cat([whole, whole, half]).contiguous(), src


def stats(xs, unit="ms"):
    return {"median_" + unit: statistics.median(xs), "min_" + unit: min(xs), "max_" + unit: max(xs)}


def timed(eng, fn, reps):
    ev, wall = [], []
    for i in range(3 + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        eng.synchronize()
        t0 = time.perf_counter()
        a.record()
        out = fn()
        b.record()
        eng.synchronize()
        torch.cuda.synchronize()
        if i >= 3:
            wall.append((time.perf_counter() - t0) * 1e3)
            ev.append(a.elapsed_time(b))
    return out, {"events": stats(ev), "wall": stats(wall)}


def laps_of(stderr):
    line = [ln for ln in stderr.splitlines() if ln.startswith("timing:") and ln.endswith(" s;")][-1]
    return {m[0]: float(m[1]) for m in re.findall(r" ([a-z+ ]+?) ([0-9.e+-]+) s;", line)}


def cli_cell(bases_host, reads_host, tmp, tag, winner, parent, runs):
    fa, pool = os.path.join(tmp, tag + ".fa"), os.path.join(tmp, tag + "_pool.fa")
    if not os.path.exists(fa + ".msh"):
        with open(fa, "wb") as f:
            for i, row in enumerate(bases_host):
                f.write(b">g%d\n" % i + row.tobytes() + b"\n")
        subprocess.run([MASH, "sketch", "-i", "-k", str(K), "-s", str(S), "-o", fa, fa], check=True, capture_output=True, timeout=300)
    with open(pool, "wb") as f:
        for i, rec in enumerate(reads_host.tobytes().split(b"\n")):
            if rec:
                f.write(b">r%d\n" % i + rec + b"\n")
    out = {"new": [], "parent": []}
    texts = {}
    for _ in range(runs):
        for who, exe in (("new", MASH), ("parent", parent)):
            r = subprocess.run([exe, "screen", *(["-w"] if winner else []), fa + ".msh", pool], capture_output=True, timeout=300,
                               env=dict(os.environ, MASH_AMD_TIMING="1"))
            assert r.returncode == 0, r.stderr[-300:]
            out[who].append(laps_of(r.stderr.decode()))
            texts[who] = r.stdout
    assert texts["new"] == texts["parent"], "the two commands print different rows"
    res = {"rows_printed": texts["new"].count(b"\n")}
    for who, tail in (("new", "results"), ("parent", "host tail")):
        res[who] = {"screen": stats([x["screen"] for x in out[who]], "s"), "tail_lap": tail, "tail": stats([x[tail] for x in out[who]], "s"),
                    "screen_plus_tail": stats([x["screen"] + x[tail] for x in out[who]], "s")}
    return res


def write(res, path):
    """one cell per line"""
    head = {k: v for k, v in res.items() if k != "cells"}
    with open(path, "w") as f:
        f.write(json.dumps(head)[:-1] + ', "cells": [\n' + ",\n".join(json.dumps(c) for c in res["cells"]) + "\n]}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--db", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent-mash", default=None)
    ap.add_argument("--cli-runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "screen_results_bench.json"))
    a = ap.parse_args()
    torch.cuda.init()
    eng = MashGpu(0, stream=torch.cuda.current_stream().cuda_stream)
    p = eng.params(k=K, s=S)
    kspace = 4.0 ** K
    res = {"k": K, "s": S, "genome_len": L, "db_sketches": a.db, "reps": a.reps, "cells": [],
           "parent_route": "measured" if a.parent_mash else "not measured in this run (no --parent-mash)"}
    tmp = tempfile.mkdtemp(prefix="screen_results_bench_")
    for name, per in (("clusters100", 100), ("clades1000", 1000)):
        bases = make_genomes(a.db, per, seed=per)
        gh = torch.empty((a.db, S), dtype=torch.int64, device="cuda")
        gn = torch.empty(a.db, dtype=torch.int32, device="cuda")
        off = np.arange(a.db + 1, dtype=np.uint64) * np.uint64(L)
        torch.cuda.synchronize()
        eng.sketch_dev(bases.data_ptr(), a.db * L, off, p, gh.data_ptr(), gn.data_ptr())
        eng.synchronize()
        lengths = torch.full((a.db,), L, dtype=torch.int64, device="cuda")
        db = eng.table_wrap(gh.data_ptr(), gn.data_ptr(), lengths.data_ptr(), a.db, S)
        bases_host = bases.cpu().numpy() if a.parent_mash else None
        with eng.screen_open(db, p) as sc:
            for frac in (0.001, 0.01, 0.1):
                reads, src = mixture(bases, per, frac)
                torch.cuda.synchronize()
                sc.add_dev(reads.data_ptr(), int(reads.numel()))
                (hits, _, _), t_sparse = timed(eng, sc.finish_sparse, a.reps)
                touched = int(len(np.unique(hits["row"])))
                for winner in (False, True):
                    (rows, _, _, _), t_new = timed(eng, lambda: sc.results(kspace, winner=winner), a.reps)
                    cell = {"db": name, "target_fraction": frac, "source_genomes": int(len(src)), "rows_touched": touched, "hits": int(len(hits)),
                            "winner": winner, "rows_out": int(len(rows)), "results": t_new, "finish_sparse": t_sparse}
                    if a.parent_mash:
                        cell["cli"] = cli_cell(bases_host, reads.cpu().numpy(), tmp, name, winner, a.parent_mash, a.cli_runs)
                    res["cells"].append(cell)
                    print(json.dumps(cell), flush=True)
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                    write(res, a.out)                                        # (after every cell: a run that is cut short keeps what it has)
                sc.reset()
        db.free()
    shutil.rmtree(tmp, ignore_errors=True)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
