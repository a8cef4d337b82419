#!/usr/bin/env python3
"""The k nearest references per query (mg_compare_rect_topk_host) beside what a caller of the library did without it:
100 000 resident references (the C3 generator, s = 1000), Q queries drawn from the same clusters, one process on one device.

    python tools/topk_bench.py [--refs 100000] [--reps 20] [--out profiles/topk_bench.json]
    python tools/topk_bench.py --only Q K      # the new call alone, filters off, --reps times (for a kernel trace)

Baseline, filters off: mg_compare_rect_pairs_host (32 B per pair to the host) + selection with numpy; with -d 0.05:
mg_compare_rect_results_host (the survivors) + selection with numpy.  The numpy selection is exact here: with denominators
<= 1000 distinct fractions differ by more than 1e-6, so the float64 quotient scaled to 2^40 is an order-isomorphic integer,
and the reference index goes into its low 17 bits.  Times are wall clock around calls that return finished host arrays (they
end in a device synchronise); every shape is warmed up; new and baseline alternate; the fetch of the baseline is timed once per
repetition and shared by the three k (its selection is timed per k).  The outputs are compared at every timed size."""
import argparse, json, os, statistics, sys, time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from workloads import synth_torch  # noqa: E402
from mash_amd.abi import MashGpu  # noqa: E402

K, S, L = 21, 1000, 1_000_000
KSPACE = 4.0 ** K
QS, KS = (1, 64, 4096), (1, 10, 100)
FILTERS = {"off": -1.0, "d0.05": 0.05}


def composite(numer, denom, col):
    q = np.rint(numer.astype(np.float64) / np.maximum(denom, 1).astype(np.float64) * float(1 << 40)).astype(np.int64)
    return (q << 17) | (131071 - col.astype(np.int64))


def select_matrix(pairs, k):
    """pairs [Q, nref] of mg_pair -> (rows, cols) of the answer"""
    nref = pairs.shape[1]
    kk = min(k, nref)
    out_r, out_c = [], []
    for r0 in range(0, pairs.shape[0], 256):                   # (blocks of rows: the keys of 256 rows are 200 MB)
        blk = pairs[r0:r0 + 256]
        comp = composite(blk["numer"], blk["denom"], np.arange(nref)[None, :])
        comp[blk["pass"] == 0] = -1
        part = np.argpartition(comp, nref - kk, axis=1)[:, nref - kk:]
        pc = np.take_along_axis(comp, part, 1)
        order = np.argsort(-pc, axis=1, kind="stable")
        cols = np.take_along_axis(part, order, 1)
        keep = np.take_along_axis(pc, order, 1) >= 0
        rows = np.broadcast_to(np.arange(r0, r0 + blk.shape[0])[:, None], cols.shape)
        out_r.append(rows[keep])
        out_c.append(cols[keep])
    return np.concatenate(out_r), np.concatenate(out_c)


def select_list(res, k):
    """survivors in reference order -> (rows, cols) of the answer"""
    comp = composite(res["numer"], res["denom"], res["col"])
    order = np.lexsort((-comp, res["row"]))
    r = res["row"][order]
    first = np.searchsorted(r, r, side="left")
    keep = np.arange(len(r)) - first < k
    return r[keep], res["col"][order][keep]


def stats(v):
    return {"median_ms": 1e3 * statistics.median(v), "min_ms": 1e3 * min(v), "max_ms": 1e3 * max(v), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--refs", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", type=int, nargs=2, default=None)
    a = ap.parse_args()
    torch.cuda.init()
    eng = MashGpu(0)
    clusters = max(1, a.refs // 100)
    rh, rn, rl = synth_torch.clustered_sketch_table(a.refs, S, clusters=clusters, device="cuda")
    qh, qn, ql = synth_torch.clustered_sketch_table(max(QS), S, clusters=clusters, seed=9, device="cuda")
    torch.cuda.synchronize()
    ref = eng.table_wrap(rh.data_ptr(), rn.data_ptr(), rl.data_ptr(), a.refs, S)
    qry = eng.table_wrap(qh.data_ptr(), qn.data_ptr(), ql.data_ptr(), max(QS), S)

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out

    if a.only:
        nq, k = a.only
        for _ in range(a.reps + 2):
            eng.compare_rect_topk(ref, qry, K, KSPACE, k, q_end=nq)
        return
    res = {"device": torch.cuda.get_device_name(0), "references": a.refs, "sketch_size": S, "repetitions": a.reps, "cells": []}
    for fname, max_d in FILTERS.items():
        for nq in QS:
            base_bytes = nq * a.refs * 32
            reps = a.reps
            fetch = (lambda: eng.compare_rect_pairs(ref, qry, K, KSPACE, q_end=nq)) if fname == "off" else \
                    (lambda: eng.compare_rect_results(ref, qry, K, KSPACE, max_d, q_end=nq))
            select = select_matrix if fname == "off" else select_list
            t_fetch, t_sel, t_new = [], {k: [] for k in KS}, {k: [] for k in KS}
            out_bytes = {}
            for rep in range(-1, reps):                        # (rep -1 warms every shape up and checks the outputs)
                dt, got = timed(fetch)
                if rep >= 0:
                    t_fetch.append(dt)
                for k in KS:
                    dn, new = timed(lambda: eng.compare_rect_topk(ref, qry, K, KSPACE, k, max_d, q_end=nq))
                    ds, (rows, cols) = timed(lambda: select(got, k))
                    if rep >= 0:
                        t_new[k].append(dn)
                        t_sel[k].append(ds)
                        continue
                    assert np.array_equal(new["row"], rows) and np.array_equal(new["col"], cols), (fname, nq, k)
                    src = got[rows, cols] if fname == "off" else None
                    if src is not None:
                        assert np.array_equal(new["distance"].view(np.uint64), src["distance"].view(np.uint64))
                        assert np.array_equal(new["p_value"].view(np.uint64), src["p_value"].view(np.uint64))
                    out_bytes[k] = int(len(new)) * 32
                if fname != "off":
                    base_bytes = int(len(got)) * 32
                del got
            for k in KS:
                base = [f + s for f, s in zip(t_fetch, t_sel[k])]
                cell = {"filter": fname, "queries": nq, "k": k, "baseline": stats(base), "baseline_fetch": stats(t_fetch),
                        "baseline_select": stats(t_sel[k]), "new": stats(t_new[k]),
                        "ratio_of_medians": statistics.median(base) / statistics.median(t_new[k]),
                        "baseline_bytes": base_bytes, "new_bytes": out_bytes[k]}
                res["cells"].append(cell)
                print(json.dumps(cell), flush=True)
    text = json.dumps(res, indent=1)
    if a.out:
        open(a.out, "w").write(text + "\n")
    print(json.dumps({"done": True, "cells": len(res["cells"])}))


if __name__ == "__main__":
    main()
