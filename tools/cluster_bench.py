#!/usr/bin/env python3
"""Single-linkage clusters on the device (mg_cluster_tri_host) beside the route a caller of the library had without it:
mg_compare_tri_results_host (count first, then fetch the records) plus a union-find over the records on the host (numpy
min-label propagation with pointer jumping), in one process on one device, at -d 0.05.

    python tools/cluster_bench.py [--reps 5] [--out profiles/cluster_bench.json]
    python tools/cluster_bench.py --only c3|species     # the new call alone, --reps times (for a kernel trace)

Tables: the C3 generator (100 000 sketches in clusters of 100, s = 1000) and one species of 32 768 sketches
(species_sketch_table).  Each is timed PER TABLE (a fresh table every repetition: the index build is inside the call) and as
FURTHER PASSES over a resident table.  If the baseline's records do not fit host memory (32 B per edge, twice: the fetch
buffer and numpy's index arrays) the species table is halved until they do, and the n used is recorded.  Times are wall clock
around calls that return finished host arrays; new and baseline alternate; labels and edge counts are compared once per table."""
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


def host_labels(n, rows, cols):
    rows = rows.astype(np.int64)
    cols = cols.astype(np.int64)
    lab = np.arange(n, dtype=np.int64)
    while True:
        m = np.minimum(lab[rows], lab[cols])
        new = lab.copy()
        np.minimum.at(new, lab[rows], m)
        np.minimum.at(new, lab[cols], m)
        np.minimum.at(new, rows, m)
        np.minimum.at(new, cols, m)
        while True:
            j = new[new]
            if np.array_equal(j, new):
                break
            new = j
        if np.array_equal(new, lab):
            return lab.astype(np.uint32)
        lab = new


def count_edges(eng, t):
    """mg_compare_tri_results_host with capacity 0: the count (MG_ERR_NOMEM is its way of saying so)"""
    import ctypes as C
    n = C.c_uint64(0)
    rc = eng.lib.mg_compare_tri_results_host(eng.ctx, t.handle, 0, t.rows, K, KSPACE, MAX_D, -1.0, None, 0, C.byref(n))
    assert rc in (abi.MG_OK, abi.MG_ERR_NOMEM), rc
    return int(n.value)


def baseline(eng, t):
    """-> labels, edges, seconds of (the counting call, the fetching call alone, the host union-find)"""
    t0 = time.perf_counter()
    n_edges = count_edges(eng, t)
    t1 = time.perf_counter()
    rec = eng.compare_tri_results(t, K, KSPACE, MAX_D, -1.0, capacity=max(n_edges, 1))
    t2 = time.perf_counter()
    lab = host_labels(t.rows, rec["row"], rec["col"])
    return lab, len(rec), (t1 - t0, t2 - t1, time.perf_counter() - t2)


def stats(v):
    return {"median_ms": 1e3 * statistics.median(v), "min_ms": 1e3 * min(v), "max_ms": 1e3 * max(v), "n": len(v)}


def summary(t_new, t_old):
    """t_old: (count, fetch, union) per repetition.  results_alone is mg_compare_tri_results_host with a buffer that fits -- on a
    fresh table it follows the counting call, which has built the index, so per table the pair count + fetch is the honest figure"""
    return {"new": stats(t_new), "baseline_count_call": stats([x[0] for x in t_old]), "baseline_results_alone": stats([x[1] for x in t_old]),
            "baseline_host_union": stats([x[2] for x in t_old]), "baseline_total": stats([sum(x) for x in t_old]),
            "new_over_results_alone": statistics.median(t_new) / statistics.median([x[1] for x in t_old]),
            "baseline_total_over_new": statistics.median([sum(x) for x in t_old]) / statistics.median(t_new)}


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
        while True:
            h, nh, ln = make(n)
            torch.cuda.synchronize()
            t = eng.table_wrap(h.data_ptr(), nh.data_ptr(), ln.data_ptr(), n, S)
            if a.only:
                break
            n_edges = count_edges(eng, t)
            if n_edges * 32 * 4 < host_room() or n <= 1024:      # records, index arrays and labels' gathers of the baseline
                break
            t.free()
            n //= 2
        if a.only:
            for _ in range(a.reps + 2):
                eng.cluster_tri_host(t, K, KSPACE, MAX_D, -1.0)
            return
        # outputs agree (and warm-up of both)
        lab_new, nc, ne = eng.cluster_tri_host(t, K, KSPACE, MAX_D, -1.0)
        lab_old, ne_old, _ = baseline(eng, t)
        assert ne == ne_old == n_edges and np.array_equal(lab_new, lab_old), (name, ne, ne_old)
        cell = {"table": name, "n": n, "edges": ne, "clusters": nc, "baseline_record_bytes": ne * 32, "new_bytes": n * 4}
        # further passes over the resident table
        t_new, t_old = [], []
        for _ in range(a.reps):
            t_new.append(timed(lambda: eng.cluster_tri_host(t, K, KSPACE, MAX_D, -1.0))[0])
            t_old.append(baseline(eng, t)[2])
        cell["further_passes"] = summary(t_new, t_old)
        # per table: a fresh table each time, so the index build is inside the first call
        t_new, t_old = [], []
        for _ in range(max(2, a.reps // 2)):
            t.invalidate()
            t_new.append(timed(lambda: eng.cluster_tri_host(t, K, KSPACE, MAX_D, -1.0))[0])
            t.invalidate()
            t_old.append(baseline(eng, t)[2])
        cell["per_table"] = summary(t_new, t_old)
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
