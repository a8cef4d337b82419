#!/usr/bin/env python3
"""The minimum spanning forest on the device (mg_cluster_tri_forest_host) beside its two neighbours of the same run, in one process
on one device, at -d 0.05:
  * mg_cluster_tri_host alone -- the FLOOR: the same compare and ballots, no edge list, no rounds, no records;
  * the only way to the same answer without it: mg_compare_tri_results_host (count first, then fetch the records, 32 bytes per
    edge) plus a stable sort by the exact fraction and Kruskal over the fetched records on the host.

    python tools/forest_bench.py [--reps 3] [--out profiles/forest_bench.json]
    python tools/forest_bench.py --only c3|species     # the new call alone, --reps times (for a kernel trace)

Tables: the C3 generator (100 000 sketches in clusters of 100, s = 1000) and one species of 32 768 sketches
(species_sketch_table).  Each is timed PER TABLE (a fresh table every repetition: the index build is inside the call) and as FURTHER
PASSES over a resident table.  Times are wall clock around calls that return finished host arrays; the calls alternate within a
repetition; medians are reported.  The host sort + Kruskal is CPU work that no repetition changes: it is timed once per table.  The
forest, the labels and the counts are compared with the baseline's once per table, before anything is timed.  No time is a condition;
what is recorded is the ratio of the new call to the floor (new_over_single_linkage) and to the fetching results call
(new_over_results_alone; the expectation is <= 1 at one species: rows - 1 records cross PCIe instead of 32 bytes per edge).
Recorded beside them: rounds, regrows, and per round the live edges it began with and the forest edges it chose
(mg_cluster_forest_rounds).  Dead-edge compaction is not built, so there is no on / off to compare."""
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


def host_forest(n, rec):
    """indices of the forest's records, best first: a stable sort of the records (they come in `triangle -E` order) by numer * 2^42
    // denom, which orders as the fraction does below 2^21, then Kruskal in chunks -- a chunk's edges whose ends already share a
    label are dropped at once, only the others are walked"""
    key = (rec["numer"].astype(np.uint64) << np.uint64(42)) // np.maximum(rec["denom"], 1).astype(np.uint64)
    order = np.argsort(~key, kind="stable")
    row, col = rec["row"].astype(np.int64), rec["col"].astype(np.int64)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    kept = []
    chunk = max(4 * n, 1024)
    for lo in range(0, len(order), chunk):
        idx = order[lo:lo + chunk]
        lab = np.array(parent, dtype=np.int64)
        while True:
            nxt = lab[lab]
            if np.array_equal(nxt, lab):
                break
            lab = nxt
        idx = idx[lab[row[idx]] != lab[col[idx]]]
        for i in idx.tolist():
            a, b = find(int(row[i])), find(int(col[i]))
            if a != b:
                parent[max(a, b)] = min(a, b)
                kept.append(i)
    return np.array(kept, dtype=np.int64)


def count_edges(eng, t):
    """mg_compare_tri_results_host with capacity 0: the count (MG_ERR_NOMEM is its way of saying so)"""
    import ctypes as C
    n = C.c_uint64(0)
    rc = eng.lib.mg_compare_tri_results_host(eng.ctx, t.handle, 0, t.rows, K, KSPACE, MAX_D, -1.0, None, 0, C.byref(n))
    assert rc in (abi.MG_OK, abi.MG_ERR_NOMEM), rc
    return int(n.value)


def baseline(eng, t):
    """-> records, seconds of (the counting call, the fetching call alone)"""
    t0 = time.perf_counter()
    n_edges = count_edges(eng, t)
    t1 = time.perf_counter()
    rec = eng.compare_tri_results(t, K, KSPACE, MAX_D, -1.0, capacity=max(n_edges, 1))
    return rec, (t1 - t0, time.perf_counter() - t1)


def stats(v):
    return {"median_ms": 1e3 * statistics.median(v), "min_ms": 1e3 * min(v), "max_ms": 1e3 * max(v), "n": len(v)}


def summary(t_new, t_single, t_old, host_s):
    """t_old: (count, fetch) per repetition.  results_alone is mg_compare_tri_results_host with a buffer that fits -- on a fresh
    table it follows the counting call, which has built the index, so per table count + fetch is the honest figure"""
    new, fetch, both = statistics.median(t_new), statistics.median([x[1] for x in t_old]), statistics.median([sum(x) for x in t_old])
    return {"new": stats(t_new), "single_linkage": stats(t_single), "baseline_count_call": stats([x[0] for x in t_old]),
            "baseline_results_alone": stats([x[1] for x in t_old]), "baseline_count_and_fetch": stats([sum(x) for x in t_old]),
            "baseline_host_sort_kruskal_ms_once": 1e3 * host_s,
            "new_over_single_linkage": new / statistics.median(t_single), "new_over_results_alone": new / fetch,
            "baseline_total_over_new": (both + host_s) / new}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=["c3", "species"], default=None)
    a = ap.parse_args()
    torch.cuda.init()
    eng = MashGpu(0)
    makers = {"c3": (100_000, lambda n: synth_torch.clustered_sketch_table(n, S, clusters=n // 100, device="cuda")),
              "species": (32_768, lambda n: synth_torch.species_sketch_table(n, S, device="cuda"))}
    res = {"device": torch.cuda.get_device_name(0), "sketch_size": S, "max_distance": MAX_D, "repetitions": a.reps, "tables": []}
    forest = lambda t: eng.cluster_tri_forest_host(t, K, KSPACE, MAX_D, -1.0)      # noqa: E731
    single = lambda t: eng.cluster_tri_host(t, K, KSPACE, MAX_D, -1.0)             # noqa: E731
    for name, (n, make) in makers.items():
        if a.only and a.only != name:
            continue
        h, nh, ln = make(n)
        torch.cuda.synchronize()
        t = eng.table_wrap(h.data_ptr(), nh.data_ptr(), ln.data_ptr(), n, S)
        if a.only:
            for _ in range(a.reps + 2):
                forest(t)
            return
        # outputs agree (and warm-up of all three)
        got, label, nc, ne = forest(t)
        st = eng.cluster_forest_stats()
        live, chosen = eng.cluster_forest_rounds()
        rec, _ = baseline(eng, t)
        host_s, kept = timed(lambda: host_forest(n, rec))
        lab_single, nc_single, ne_single = single(t)
        assert ne == len(rec) == ne_single and nc == nc_single and np.array_equal(label, lab_single), (name, ne, len(rec), ne_single)
        assert got.tobytes() == rec[kept].tobytes() and len(got) == n - nc, name
        del rec, kept
        cell = {"table": name, "n": n, "edges": ne, "clusters": nc, "forest_edges": len(got), "rounds": st["rounds"], "rounds_bound": n.bit_length(),
                "live_edges_per_round": live, "chosen_per_round": chosen, "regrows": st["regrows"], "edge_capacity": st["edge_capacity"], "outputs_equal_baseline": True,
                "baseline_record_bytes": ne * 32, "new_bytes": len(got) * 32 + n * 4, "device_edge_list_bytes": st["edge_capacity"] * 16}
        # further passes over the resident table
        t_new, t_single, t_old = [], [], []
        for _ in range(a.reps):
            t_new.append(timed(lambda: forest(t))[0])
            t_old.append(baseline(eng, t)[1])
            t_single.append(timed(lambda: single(t))[0])
        cell["further_passes"] = summary(t_new, t_single, t_old, host_s)
        # per table: a fresh table each time, so the index build is inside the first call
        t_new, t_single, t_old = [], [], []
        for _ in range(max(2, a.reps // 2)):
            t.invalidate()
            t_new.append(timed(lambda: forest(t))[0])
            t.invalidate()
            t_old.append(baseline(eng, t)[1])
            t.invalidate()
            t_single.append(timed(lambda: single(t))[0])
        cell["per_table"] = summary(t_new, t_single, t_old, host_s)
        res["tables"].append(cell)
        print(json.dumps(cell), flush=True)
        t.free()
        del h, nh, ln
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    print(json.dumps({"done": True, "tables": len(res["tables"])}))


if __name__ == "__main__":
    main()
