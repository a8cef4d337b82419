#!/usr/bin/env python3
"""The k nearest neighbours of every sketch of one table (mg_compare_tri_topk_host) beside the two routes a caller of the library
had without it, in one process on one device, at -d 0.05:

  results  mg_compare_tri_results_host (count first, then fetch the records) plus a numpy symmetrise-and-select on the host;
  rect     mg_compare_rect_topk_host of the table against itself with k + 1 (every pair compared twice, each sketch its own
           nearest neighbour: dropped on the host).

    python tools/knn_bench.py [--reps 5] [--species 32768] [--out profiles/knn_bench.json]
    python tools/knn_bench.py --only c3|species K     # the new call alone, --reps times (for a kernel trace)

Tables: the C3 generator (100 000 sketches in clusters of 100, s = 1000) and one species of 32 768 sketches
(species_sketch_table); k in {1, 10, 100}.  Each is timed as FURTHER PASSES over a resident table and PER TABLE (a fresh table
every repetition: the index build is inside the call).  If the records of `results` do not fit host memory the species table is
halved until they do, and the n used is recorded.  The numpy selection is exact here: with denominators <= 1000 distinct
fractions differ by more than 1e-6, so the float64 quotient scaled to 2^40 is an order-isomorphic integer, and the neighbour
index goes into its low 17 bits.  Times are wall clock around calls that return finished host arrays (they end in a device
synchronise); the three routes alternate; the outputs are compared once per table and k, before anything is timed."""
import argparse, ctypes as C, json, os, statistics, sys, time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from workloads import synth_torch  # noqa: E402
from mash_amd import abi  # noqa: E402
from mash_amd.abi import MashGpu  # noqa: E402

K, S = 21, 1000
KSPACE = 4.0 ** K
MAX_D = 0.05
KS = (1, 10, 100)


def count_edges(eng, t):
    """mg_compare_tri_results_host with capacity 0: the count (MG_ERR_NOMEM is its way of saying so)"""
    n = C.c_uint64(0)
    rc = eng.lib.mg_compare_tri_results_host(eng.ctx, t.handle, 0, t.rows, K, KSPACE, MAX_D, -1.0, None, 0, C.byref(n))
    assert rc in (abi.MG_OK, abi.MG_ERR_NOMEM), rc
    return int(n.value)


def select(rows, nbr, numer, denom, k):
    """(row, neighbour) of every row's first k entries, rows ascending, best first, equal fractions by neighbour"""
    q = np.rint(numer.astype(np.float64) / np.maximum(denom, 1).astype(np.float64) * float(1 << 40)).astype(np.int64)
    comp = (q << 17) | (131071 - nbr.astype(np.int64))
    order = np.lexsort((-comp, rows))
    r = rows[order]
    keep = np.arange(len(r)) - np.searchsorted(r, r, side="left") < k
    return r[keep], nbr[order][keep]


def via_results(eng, t, k):
    """-> (rows, neighbours), records, seconds of (the counting call, the fetching call, the host selection)"""
    t0 = time.perf_counter()
    n_edges = count_edges(eng, t)
    t1 = time.perf_counter()
    rec = eng.compare_tri_results(t, K, KSPACE, MAX_D, -1.0, capacity=max(n_edges, 1))
    t2 = time.perf_counter()
    out = select(np.concatenate([rec["row"], rec["col"]]), np.concatenate([rec["col"], rec["row"]]), np.concatenate([rec["numer"]] * 2),
                 np.concatenate([rec["denom"]] * 2), k)
    return out, len(rec), (t1 - t0, t2 - t1, time.perf_counter() - t2)


def via_rect(eng, t, k):
    """-> (rows, neighbours), seconds of (the call, dropping self on the host)"""
    t0 = time.perf_counter()
    rec = eng.compare_rect_topk(t, t, K, KSPACE, k + 1, MAX_D)
    t1 = time.perf_counter()
    rec = rec[rec["row"] != rec["col"]]
    r = rec["row"]
    keep = np.arange(len(r)) - np.searchsorted(r, r, side="left") < k
    return (r[keep], rec["col"][keep]), (t1 - t0, time.perf_counter() - t1)


def stats(v):
    return {"median_ms": 1e3 * statistics.median(v), "min_ms": 1e3 * min(v), "max_ms": 1e3 * max(v), "n": len(v)}


def summary(t_new, t_res, t_rect):
    return {"new": stats(t_new), "results_count_call": stats([x[0] for x in t_res]), "results_fetch_call": stats([x[1] for x in t_res]),
            "results_host_select": stats([x[2] for x in t_res]), "results_total": stats([sum(x) for x in t_res]),
            "rect_call": stats([x[0] for x in t_rect]), "rect_total": stats([sum(x) for x in t_rect]),
            "results_total_over_new": statistics.median([sum(x) for x in t_res]) / statistics.median(t_new),
            "rect_total_over_new": statistics.median([sum(x) for x in t_rect]) / statistics.median(t_new)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def host_room():
    for ln in open("/proc/meminfo"):
        if ln.startswith("MemAvailable:"):
            return int(ln.split()[1]) * 1024
    return 1 << 36


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--species", type=int, default=32_768, help="sketches of the species table (the host selection of `results` sorts two entries per edge)")
    ap.add_argument("--only", nargs=2, default=None, metavar=("TABLE", "K"))
    a = ap.parse_args()
    torch.cuda.init()
    eng = MashGpu(0)
    makers = {"c3": (100_000, lambda n: synth_torch.clustered_sketch_table(n, S, clusters=n // 100, device="cuda")),
              "species": (a.species, lambda n: synth_torch.species_sketch_table(n, S, device="cuda"))}
    if a.only and a.only[0] not in makers:
        ap.error("--only takes c3 or species and a k")
    res = {"device": torch.cuda.get_device_name(0), "sketch_size": S, "max_distance": MAX_D, "repetitions": a.reps, "cells": []}
    for name, (n, make) in makers.items():
        if a.only and a.only[0] != name:
            continue
        while True:
            h, nh, ln = make(n)
            torch.cuda.synchronize()
            t = eng.table_wrap(h.data_ptr(), nh.data_ptr(), ln.data_ptr(), n, S)
            if a.only:
                break
            n_edges = count_edges(eng, t)
            if n_edges * 32 * 6 < host_room() or n <= 1024:       # the records, their mirrored copies and the sort's index arrays
                break
            t.free()
            n //= 2
        if a.only:
            for _ in range(a.reps + 2):
                eng.compare_tri_topk(t, K, KSPACE, int(a.only[1]), MAX_D)
            return
        for k in KS:
            # outputs agree (and warm-up of all three)
            new = eng.compare_tri_topk(t, K, KSPACE, k, MAX_D)
            (rr, rc), ne, _ = via_results(eng, t, k)
            (qr, qc), _ = via_rect(eng, t, k)
            assert np.array_equal(new["row"], rr) and np.array_equal(new["col"], rc), (name, k, "results")
            assert np.array_equal(new["row"], qr) and np.array_equal(new["col"], qc), (name, k, "rect")
            cell = {"table": name, "n": n, "k": k, "edges": ne, "records": int(len(new)), "results_record_bytes": ne * 32, "new_bytes": int(len(new)) * 32}
            t_new, t_res, t_rect = [], [], []
            for _ in range(a.reps):                                # further passes over the resident table
                t_new.append(timed(lambda: eng.compare_tri_topk(t, K, KSPACE, k, MAX_D))[0])
                t_res.append(via_results(eng, t, k)[2])
                t_rect.append(via_rect(eng, t, k)[1])
            cell["further_passes"] = summary(t_new, t_res, t_rect)
            t_new, t_res, t_rect = [], [], []
            for _ in range(max(2, a.reps // 2)):                   # per table: a fresh table each time, the index build inside the call
                t.invalidate()
                t_new.append(timed(lambda: eng.compare_tri_topk(t, K, KSPACE, k, MAX_D))[0])
                t.invalidate()
                t_res.append(via_results(eng, t, k)[2])
                t.invalidate()
                t_rect.append(via_rect(eng, t, k)[1])
            cell["per_table"] = summary(t_new, t_res, t_rect)
            res["cells"].append(cell)
            print(json.dumps(cell), flush=True)
        t.free()
        del h, nh, ln
    text = json.dumps(res, indent=1)
    if a.out:
        open(a.out, "w").write(text + "\n")
    print(json.dumps({"done": True, "cells": len(res["cells"])}))


if __name__ == "__main__":
    main()
