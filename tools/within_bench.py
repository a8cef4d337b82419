#!/usr/bin/env python3
"""`mash within` on the device (mg_within_rect_results_host) beside what a caller did without it, on resident synthetic tables
(workloads/synth_torch.containment_tables), one process on one device.

    python tools/within_bench.py [--queries 10000] [--reps 5] [--out profiles/within_bench.json]
    python tools/within_bench.py --only refs1000 e0.05      # the thresholded call alone, --reps times (for a kernel trace)

Jobs: `refs1000` -- 1 000 references of s = 10 000 x the queries of s = 1 000 --, `ref1` -- one reference of s = 100 000 x the same
number of queries; each at -e 0.05 and unfiltered (-e 1).  A query is a contig of one reference covering 2 % or 5 % of it, so at
-e 0.05 (j >= 400) the 2 % contigs drop out by their j and the 5 % contigs survive against EVERY reference: j depends on the
value ranges alone, the shared count is what tells the home reference from the others.
Timed, alternating, every shape warmed up:
  new       mg_within_rect_results_host
  full      mg_within_rect_host + a numpy filter of its output (what a user did without the device filter)
  compare   mg_compare_rect_results_host -d 0.05 on the same tables (the existing job of the same shape)
and the model's serial walk (tests/within_model.py) on a sample of pairs, as a CPU rate.  Before anything is timed the device's
{common, j} is compared with the model on a seeded sample of pairs, and `new` with the filtered `full`."""
import argparse, json, math, os, statistics, sys, time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from workloads import synth_torch  # noqa: E402
from mash_amd.abi import MashGpu  # noqa: E402
from tests import within_model as wm  # noqa: E402

K, KSPACE = 21, 4.0 ** 21
JOBS = {"refs1000": (1000, 10_000), "ref1": (1, 100_000)}
ERRORS = {"e0.05": wm.as_float(0.05), "e1": 1.0}
S_QRY = 1000


def stats(v):
    return {"median_ms": 1e3 * statistics.median(v), "min_ms": 1e3 * min(v), "max_ms": 1e3 * max(v), "n": len(v)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", nargs=2, default=None)
    a = ap.parse_args()
    torch.cuda.init()
    eng = MashGpu(0)
    res = {"device": torch.cuda.get_device_name(0), "queries": a.queries, "query_sketch_size": S_QRY, "repetitions": a.reps, "cells": []}
    for job, (nref, s_ref) in JOBS.items():
        if a.only and a.only[0] != job:
            continue
        (rh, rn, rl), (qh, qn, ql) = synth_torch.containment_tables(nref, s_ref, a.queries, S_QRY, seed=1)
        torch.cuda.synchronize()
        ref = eng.table_wrap(rh.data_ptr(), rn.data_ptr(), rl.data_ptr(), nref, s_ref)
        qry = eng.table_wrap(qh.data_ptr(), qn.data_ptr(), ql.data_ptr(), a.queries, S_QRY)
        if a.only:
            for _ in range(a.reps + 1):
                eng.within_rect_results(ref, qry, ERRORS[a.only[1]], capacity=1 << 24)
            continue
        # the device against the model on a seeded sample of pairs, and the model's walk as a CPU rate
        rng = np.random.default_rng(20261021)
        qs = np.unique(np.concatenate([rng.integers(0, a.queries, 8), np.arange(4)]))
        t_walk, walked = 0.0, 0
        for q in qs:
            got = eng.within_rect_host(ref, qry, int(q), int(q) + 1)[0]
            Q = [int(x) for x in qh[int(q)].cpu().numpy().view(np.uint64)]
            for r in np.unique(np.concatenate([rng.integers(0, nref, a.sample // len(qs)), [int(q) % nref]])):
                R = [int(x) for x in rh[int(r)].cpu().numpy().view(np.uint64)]
                dt, want = timed(lambda: wm.walk(R, Q))
                t_walk += dt
                walked += 1
                assert tuple(got[int(r)]) == want, (job, int(q), int(r), tuple(got[int(r)]), want)
        for ename, e in ERRORS.items():
            t_new, t_full, t_cmp = [], [], []
            n_out = n_cmp = 0
            for rep in range(-1, a.reps):                              # (rep -1 warms up and checks)
                dn, new = timed(lambda: eng.within_rect_results(ref, qry, e, capacity=1 << 24))

                def full():
                    m = eng.within_rect_host(ref, qry)
                    j = m["denom"]
                    keep = (j >= 1) & (1.0 / np.sqrt(np.maximum(j, 1).astype(np.float64)) <= e)
                    rows, cols = np.nonzero(keep)
                    return rows, cols, m[rows, cols]
                df, (rows, cols, picked) = timed(full)
                dc, cmp_ = timed(lambda: eng.compare_rect_results(ref, qry, K, KSPACE, 0.05))
                if rep < 0:
                    assert np.array_equal(new["row"], rows) and np.array_equal(new["col"], cols)
                    assert np.array_equal(new["numer"], picked["numer"]) and np.array_equal(new["denom"], picked["denom"])
                    n_out, n_cmp = int(len(new)), int(len(cmp_))
                    continue
                t_new.append(dn); t_full.append(df); t_cmp.append(dc)
            cell = {"job": job, "references": nref, "reference_sketch_size": s_ref, "error": ename, "pairs": nref * a.queries, "survivors": n_out,
                    "new": stats(t_new), "full_plus_numpy_filter": stats(t_full), "compare_results_d0.05": stats(t_cmp), "compare_survivors": n_cmp,
                    "pairs_per_s_new": nref * a.queries / statistics.median(t_new),
                    "model_walk_pairs_per_s_cpu": walked / t_walk, "model_walk_pairs": walked}
            res["cells"].append(cell)
            print(json.dumps(cell), flush=True)
        ref.free()
        qry.free()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(res, indent=1) + "\n")
    print(json.dumps({"done": True, "cells": len(res["cells"])}))


if __name__ == "__main__":
    main()
