#!/usr/bin/env python3
"""Greedy representative clusters on the device (mg_cluster_tri_greedy_host) beside the only way to the same answer without
it: mg_compare_tri_results_host (count first, then fetch the records, 32 bytes per edge) plus the greedy walk over the fetched
records on the host, in one process on one device, at -d 0.05; mg_cluster_tri_host (single linkage) is timed beside them.

    python tools/cluster_greedy_bench.py [--reps 5] [--out profiles/cluster_greedy_bench.json]
    python tools/cluster_greedy_bench.py --only c3|species     # the new call alone, --reps times (for a kernel trace)

Tables: the C3 generator (100 000 sketches in clusters of 100, s = 1000) and one species of 32 768 sketches
(species_sketch_table).  Each is timed PER TABLE (a fresh table every repetition: the index build is inside the call) and as
FURTHER PASSES over a resident table.  Times are wall clock around calls that return finished host arrays; the calls alternate
within a repetition; medians are reported.  rep and the edge count are compared with the baseline's once per table, before
anything is timed.  The acceptance condition: on a resident table the new call is not slower than the FETCHING
mg_compare_tri_results_host call alone (new_over_results_alone <= 1)."""
import argparse, json, os, statistics, sys, time

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


def host_walk(n, rows, cols):
    """the greedy walk in index order over fetched records: edges sorted by their larger end, then row after row"""
    rows = rows.astype(np.int64)
    cols = cols.astype(np.int64)
    hi, lo = np.maximum(rows, cols), np.minimum(rows, cols)
    order = np.argsort(hi, kind="stable")
    hi, lo = hi[order], lo[order]
    start = np.searchsorted(hi, np.arange(n + 1))
    is_rep = np.zeros(n, dtype=bool)
    rep = np.arange(n, dtype=np.uint32)
    for i in range(n):
        nb = lo[start[i]:start[i + 1]]
        r = nb[is_rep[nb]] if len(nb) else nb
        if len(r):
            rep[i] = r.min()
        else:
            is_rep[i] = True
    return rep


def count_edges(eng, t):
    """mg_compare_tri_results_host with capacity 0: the count (MG_ERR_NOMEM is its way of saying so)"""
    import ctypes as C
    n = C.c_uint64(0)
    rc = eng.lib.mg_compare_tri_results_host(eng.ctx, t.handle, 0, t.rows, K, KSPACE, MAX_D, -1.0, None, 0, C.byref(n))
    assert rc in (abi.MG_OK, abi.MG_ERR_NOMEM), rc
    return int(n.value)


def baseline(eng, t):
    """-> rep, edges, seconds of (the counting call, the fetching call alone, the host walk)"""
    t0 = time.perf_counter()
    n_edges = count_edges(eng, t)
    t1 = time.perf_counter()
    rec = eng.compare_tri_results(t, K, KSPACE, MAX_D, -1.0, capacity=max(n_edges, 1))
    t2 = time.perf_counter()
    rep = host_walk(t.rows, rec["row"], rec["col"])
    return rep, len(rec), (t1 - t0, t2 - t1, time.perf_counter() - t2)


def stats(v):
    return {"median_ms": 1e3 * statistics.median(v), "min_ms": 1e3 * min(v), "max_ms": 1e3 * max(v), "n": len(v)}


def summary(t_new, t_single, t_old):
    """t_old: (count, fetch, walk) per repetition.  results_alone is mg_compare_tri_results_host with a buffer that fits -- on a
    fresh table it follows the counting call, which has built the index, so per table count + fetch is the honest figure"""
    fetch = statistics.median([x[1] for x in t_old])
    return {"new": stats(t_new), "single_linkage": stats(t_single), "baseline_count_call": stats([x[0] for x in t_old]),
            "baseline_results_alone": stats([x[1] for x in t_old]), "baseline_host_walk": stats([x[2] for x in t_old]),
            "baseline_total": stats([sum(x) for x in t_old]),
            "new_over_results_alone": statistics.median(t_new) / fetch,
            "new_over_single_linkage": statistics.median(t_new) / statistics.median(t_single),
            "baseline_total_over_new": statistics.median([sum(x) for x in t_old]) / statistics.median(t_new)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=["c3", "species"], default=None)
    a = ap.parse_args()
    torch.cuda.init()
    eng = MashGpu(0)
    makers = {"c3": (100_000, lambda n: synth_torch.clustered_sketch_table(n, S, clusters=n // 100, device="cuda")),
              "species": (32_768, lambda n: synth_torch.species_sketch_table(n, S, device="cuda"))}
    res = {"device": torch.cuda.get_device_name(0), "sketch_size": S, "max_distance": MAX_D, "repetitions": a.reps, "tables": []}
    for name, (n, make) in makers.items():
        if a.only and a.only != name:
            continue
        h, nh, ln = make(n)
        torch.cuda.synchronize()
        t = eng.table_wrap(h.data_ptr(), nh.data_ptr(), ln.data_ptr(), n, S)
        if a.only:
            for _ in range(a.reps + 2):
                eng.cluster_tri_greedy_host(t, K, KSPACE, MAX_D, -1.0)
            return
        # outputs agree (and warm-up of all three)
        rep_new, nc, ne = eng.cluster_tri_greedy_host(t, K, KSPACE, MAX_D, -1.0)
        st = eng.cluster_greedy_stats()
        rep_old, ne_old, _ = baseline(eng, t)
        _, nc_single, ne_single = eng.cluster_tri_host(t, K, KSPACE, MAX_D, -1.0)
        assert ne == ne_old == ne_single and np.array_equal(rep_new, rep_old), (name, ne, ne_old, ne_single)
        assert nc == int((rep_old == np.arange(n)).sum())
        cell = {"table": name, "n": n, "edges": ne, "clusters": nc, "single_linkage_clusters": nc_single, "rounds": st["rounds"],
                "batches": st["batches"], "regrows": st["regrows"], "edge_capacity": st["edge_capacity"], "outputs_equal_baseline": True,
                "baseline_record_bytes": ne * 32, "new_bytes": n * 4}
        # further passes over the resident table
        t_new, t_single, t_old = [], [], []
        for _ in range(a.reps):
            t_new.append(timed(lambda: eng.cluster_tri_greedy_host(t, K, KSPACE, MAX_D, -1.0))[0])
            t_old.append(baseline(eng, t)[2])
            t_single.append(timed(lambda: eng.cluster_tri_host(t, K, KSPACE, MAX_D, -1.0))[0])
        cell["further_passes"] = summary(t_new, t_single, t_old)
        # per table: a fresh table each time, so the index build is inside the first call
        t_new, t_single, t_old = [], [], []
        for _ in range(max(2, a.reps // 2)):
            t.invalidate()
            t_new.append(timed(lambda: eng.cluster_tri_greedy_host(t, K, KSPACE, MAX_D, -1.0))[0])
            t.invalidate()
            t_old.append(baseline(eng, t)[2])
            t.invalidate()
            t_single.append(timed(lambda: eng.cluster_tri_host(t, K, KSPACE, MAX_D, -1.0))[0])
        cell["per_table"] = summary(t_new, t_single, t_old)
        cell["accepted"] = cell["further_passes"]["new_over_results_alone"] <= 1.0
        res["tables"].append(cell)
        print(json.dumps(cell), flush=True)
        t.free()
        del h, nh, ln
    text = json.dumps(res, indent=1)
    if a.out:
        open(a.out, "w").write(text + "\n")
    print(json.dumps({"done": True, "tables": len(res["tables"])}))


if __name__ == "__main__":
    main()
