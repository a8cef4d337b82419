#!/usr/bin/env python3
"""Extending an earlier clustering on the device (mg_cluster_extend_host, mg_cluster_extend_greedy_host) beside what a user runs
without it: mg_cluster_tri_host / mg_cluster_tri_greedy_host on the concatenated table, in one process on one device, at -d 0.05.

    python tools/cluster_extend_bench.py [--reps 5] [--out profiles/cluster_extend_bench.json]
    python tools/cluster_extend_bench.py --only c3|species [--m 1000]     # the new calls alone, --reps times (for a kernel trace)

Tables: the C3 generator (100 000 sketches in 1 000 clusters, s = 1000) as ref with m in {100, 1 000, 10 000} new sketches drawn
from the same generator (the rows behind the first 100 000: they fall into the same clusters), and one species with 32 768
sketches as ref and m in {100, 1 000}.  The earlier result is the whole-table call on ref.  Each cell is timed PER TABLE (fresh
tables every repetition: the index builds are inside the calls) and as FURTHER PASSES with ref, qry and the concatenation
resident and indexed.  Times are wall clock around calls that return finished host arrays; the calls alternate within a
repetition; medians are reported.  Checking comes first: label, rep, the cluster counts and edges(ref) + new edges == edges(cat)
are compared with the baseline's before anything is timed.  No rate is promised: the expectation to test is that the cost follows
the pairs that touch a new row, n m + m^2 / 2, and not the (n + m)^2 / 2 of the baseline (pairs_new_over_all per cell)."""
import argparse, json, os, statistics, sys, time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from workloads import synth_torch  # noqa: E402
from mash_amd.abi import MashGpu  # noqa: E402

K, S = 21, 1000
KSPACE = 4.0 ** K
MAX_D = 0.05


def stats(v):
    return {"median_ms": 1e3 * statistics.median(v), "min_ms": 1e3 * min(v), "max_ms": 1e3 * max(v), "n": len(v)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def summary(t):
    out = {k: stats(v) for k, v in t.items()}
    out["baseline_over_new"] = statistics.median(t["baseline"]) / statistics.median(t["new"])
    out["baseline_greedy_over_new_greedy"] = statistics.median(t["baseline_greedy"]) / statistics.median(t["new_greedy"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=["c3", "species"], default=None)
    ap.add_argument("--m", type=int, default=1000)
    a = ap.parse_args()
    torch.cuda.init()
    eng = MashGpu(0)
    makers = {"c3": (100_000, (100, 1_000, 10_000), lambda rows: synth_torch.clustered_sketch_table(rows, S, clusters=1000, device="cuda")),
              "species": (32_768, (100, 1_000), lambda rows: synth_torch.species_sketch_table(rows, S, device="cuda"))}
    res = {"device": torch.cuda.get_device_name(0), "sketch_size": S, "max_distance": MAX_D, "repetitions": a.reps, "cells": []}
    for name, (n, ms, make) in makers.items():
        if a.only and a.only != name:
            continue
        for m in ((a.m,) if a.only else ms):
            h, nh, ln = make(n + m)
            torch.cuda.synchronize()
            cat = eng.table_wrap(h.data_ptr(), nh.data_ptr(), ln.data_ptr(), n + m, S)
            ref = eng.table_wrap(h.data_ptr(), nh.data_ptr(), ln.data_ptr(), n, S)
            qry = eng.table_wrap(h[n:].data_ptr(), nh[n:].data_ptr(), ln[n:].data_ptr(), m, S)
            lab_ref, nc_ref, ne_ref = eng.cluster_tri_host(ref, K, KSPACE, MAX_D, -1.0)
            rep_ref, ncg_ref, _ = eng.cluster_tri_greedy_host(ref, K, KSPACE, MAX_D, -1.0)
            calls = {"new": lambda: eng.cluster_extend_host(ref, qry, lab_ref, K, KSPACE, MAX_D, -1.0),
                     "baseline": lambda: eng.cluster_tri_host(cat, K, KSPACE, MAX_D, -1.0),
                     "new_greedy": lambda: eng.cluster_extend_greedy_host(ref, qry, rep_ref, K, KSPACE, MAX_D, -1.0),
                     "baseline_greedy": lambda: eng.cluster_tri_greedy_host(cat, K, KSPACE, MAX_D, -1.0)}
            if a.only:
                for _ in range(a.reps + 2):
                    calls["new"]()
                    calls["new_greedy"]()
                return
            # outputs agree (and warm-up of all four)
            lab, nc, ne = calls["new"]()
            lab_cat, nc_cat, ne_cat = calls["baseline"]()
            rep, ncg, neg = calls["new_greedy"]()
            st = eng.cluster_greedy_stats()
            rep_cat, ncg_cat, _ = calls["baseline_greedy"]()
            assert np.array_equal(lab, lab_cat) and nc == nc_cat and ne_ref + ne == ne_cat, (name, m, nc, nc_cat, ne_ref, ne, ne_cat)
            assert np.array_equal(rep, rep_cat[n:]) and np.array_equal(rep_ref, rep_cat[:n]) and ncg == ncg_cat and neg == ne, (name, m, ncg, ncg_cat)
            cell = {"table": name, "n": n, "m": m, "edges_ref": ne_ref, "edges_new": ne, "edges_cat": ne_cat, "clusters_ref": nc_ref, "clusters": nc,
                    "representatives_ref": ncg_ref, "representatives": ncg, "greedy_rounds": st["rounds"], "greedy_regrows": st["regrows"],
                    "outputs_equal_baseline": True,
                    "pairs_new_over_all": (n * m + m * (m - 1) / 2) / ((n + m) * (n + m - 1) / 2)}
            # further passes: every table resident and indexed
            t = {k: [] for k in calls}
            for _ in range(a.reps):
                for k, fn in calls.items():
                    t[k].append(timed(fn)[0])
            cell["further_passes"] = summary(t)
            # per table: fresh tables each time, so the index builds are inside the call
            t = {k: [] for k in calls}
            for _ in range(a.reps):
                for k, fn in calls.items():
                    for x in (cat, ref, qry):
                        x.invalidate()
                    t[k].append(timed(fn)[0])
            cell["per_table"] = summary(t)
            res["cells"].append(cell)
            print(json.dumps(cell), flush=True)
            for x in (cat, ref, qry):
                x.free()
            del h, nh, ln
    text = json.dumps(res, indent=1)
    if a.out:
        open(a.out, "w").write(text + "\n")
    print(json.dumps({"done": True, "cells": len(res["cells"])}))


if __name__ == "__main__":
    main()
