#!/usr/bin/env python3
"""Members under their NEAREST representative on the device (mg_cluster_tri_nearest_host, `mash cluster -B`) beside
  - mg_cluster_tri_greedy_host (`mash cluster -R`): the floor -- the same compare, ballots and rounds, 8 bytes an edge instead of
    16, one pass over the list behind the rounds instead of two;
  - the only way to the same answer without it: mg_compare_tri_results_host (count first, then fetch the records, 32 bytes per
    edge) plus the greedy walk and the assignment over the fetched records in numpy,
in one process on one device, at -d 0.05.

    python tools/cluster_nearest_bench.py [--reps 5] [--out profiles/cluster_nearest_bench.json]
    python tools/cluster_nearest_bench.py --only c3|species     # the new call alone, --reps times (for a kernel trace)

Tables: the C3 generator (100 000 sketches in clusters of 100, s = 1000) and one species of 32 768 sketches
(species_sketch_table).  Each is timed PER TABLE (a fresh table every repetition: the index build is inside the call) and as
FURTHER PASSES over a resident table.  Times are wall clock around calls that return finished host arrays; the calls alternate
within a repetition; medians are reported.  rep, the clusters and the edge count are compared with the numpy result once per
table, BEFORE anything is timed.  Recorded beside the times: how many members the two rules place differently, and how many are
taken by a representative later in the input.  No target time: what is measured is the extra over -R in the same process
(extra_over_greedy_ms), which should be two reads of the list and eight more bytes an edge in the append and the rounds."""
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
    """the greedy walk in index order over fetched records: edges sorted by their larger end, then row after row -> is_rep"""
    hi, lo = np.maximum(rows, cols), np.minimum(rows, cols)
    order = np.argsort(hi, kind="stable")
    hi, lo = hi[order], lo[order]
    start = np.searchsorted(hi, np.arange(n + 1))
    is_rep = np.zeros(n, dtype=bool)
    first = np.arange(n, dtype=np.uint32)
    for i in range(n):
        nb = lo[start[i]:start[i + 1]]
        r = nb[is_rep[nb]] if len(nb) else nb
        if len(r):
            first[i] = r.min()
        else:
            is_rep[i] = True
    return is_rep, first


def host_assign(n, rec):
    """walk, then every member under the representative with the best edge: the 64-bit key of forest_key.h (exact below 2^21),
    ties to the smaller representative -> rep, first (the walk's own assignment)"""
    rows, cols = rec["row"].astype(np.int64), rec["col"].astype(np.int64)
    is_rep, first = host_walk(n, rows, cols)
    keep = is_rep[rows] != is_rep[cols]
    rows, cols = rows[keep], cols[keep]
    numer, denom = rec["numer"][keep].astype(np.uint64), rec["denom"][keep].astype(np.uint64)
    member = np.where(is_rep[rows], cols, rows)
    centre = np.where(is_rep[rows], rows, cols)
    key = (numer << np.uint64(42)) // np.maximum(denom, np.uint64(1))
    order = np.lexsort((centre, np.iinfo(np.uint64).max - key, member))
    member, centre = member[order], centre[order]
    lead = np.ones(len(member), dtype=bool)
    lead[1:] = member[1:] != member[:-1]
    rep = np.arange(n, dtype=np.uint32)
    rep[member[lead]] = centre[lead]
    return rep, first


def count_edges(eng, t):
    """mg_compare_tri_results_host with capacity 0: the count (MG_ERR_NOMEM is its way of saying so)"""
    import ctypes as C
    n = C.c_uint64(0)
    rc = eng.lib.mg_compare_tri_results_host(eng.ctx, t.handle, 0, t.rows, K, KSPACE, MAX_D, -1.0, None, 0, C.byref(n))
    assert rc in (abi.MG_OK, abi.MG_ERR_NOMEM), rc
    return int(n.value)


def baseline(eng, t):
    """-> rep, first, edges, seconds of (the counting call, the fetching call alone, the numpy walk and assignment)"""
    t0 = time.perf_counter()
    n_edges = count_edges(eng, t)
    t1 = time.perf_counter()
    rec = eng.compare_tri_results(t, K, KSPACE, MAX_D, -1.0, capacity=max(n_edges, 1))
    t2 = time.perf_counter()
    rep, first = host_assign(t.rows, rec)
    return rep, first, len(rec), (t1 - t0, t2 - t1, time.perf_counter() - t2)


def stats(v):
    return {"median_ms": 1e3 * statistics.median(v), "min_ms": 1e3 * min(v), "max_ms": 1e3 * max(v), "n": len(v)}


def summary(t_new, t_greedy, t_old):
    """t_old: (count, fetch, numpy) per repetition"""
    new, greedy = statistics.median(t_new), statistics.median(t_greedy)
    return {"new": stats(t_new), "greedy": stats(t_greedy), "baseline_count_call": stats([x[0] for x in t_old]),
            "baseline_results_alone": stats([x[1] for x in t_old]), "baseline_host_walk_and_assign": stats([x[2] for x in t_old]),
            "baseline_total": stats([sum(x) for x in t_old]),
            "extra_over_greedy_ms": 1e3 * (new - greedy), "new_over_greedy": new / greedy,
            "new_over_results_alone": new / statistics.median([x[1] for x in t_old]),
            "baseline_total_over_new": statistics.median([sum(x) for x in t_old]) / new}


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
                eng.cluster_tri_nearest_host(t, K, KSPACE, MAX_D, -1.0)
            return
        # outputs agree (and warm-up of all three) before anything is timed
        rep_new, nc, ne = eng.cluster_tri_nearest_host(t, K, KSPACE, MAX_D, -1.0)
        st = eng.cluster_greedy_stats()
        rep_old, first_old, ne_old, _ = baseline(eng, t)
        rep_greedy, nc_greedy, ne_greedy = eng.cluster_tri_greedy_host(t, K, KSPACE, MAX_D, -1.0)
        st_greedy = eng.cluster_greedy_stats()
        assert ne == ne_old == ne_greedy and np.array_equal(rep_new, rep_old), (name, ne, ne_old, ne_greedy, int((rep_new != rep_old).sum()))
        assert np.array_equal(rep_greedy, first_old) and nc == nc_greedy == int((rep_old == np.arange(n)).sum())
        cell = {"table": name, "n": n, "edges": ne, "clusters": nc, "rounds": st["rounds"], "greedy_rounds": st_greedy["rounds"],
                "batches": st["batches"], "regrows": st["regrows"], "edge_capacity": st["edge_capacity"], "outputs_equal_baseline": True,
                "members_placed_differently": int((rep_new != rep_greedy).sum()),
                "members_under_a_later_representative": int((rep_new > np.arange(n)).sum()),
                "list_bytes": ne * 16, "greedy_list_bytes": ne * 8, "baseline_record_bytes": ne * 32, "new_bytes": n * 4}
        # further passes over the resident table
        t_new, t_greedy, t_old = [], [], []
        for _ in range(a.reps):
            t_new.append(timed(lambda: eng.cluster_tri_nearest_host(t, K, KSPACE, MAX_D, -1.0))[0])
            t_greedy.append(timed(lambda: eng.cluster_tri_greedy_host(t, K, KSPACE, MAX_D, -1.0))[0])
            t_old.append(baseline(eng, t)[3])
        cell["further_passes"] = summary(t_new, t_greedy, t_old)
        # per table: a fresh table each time, so the index build is inside the first call
        t_new, t_greedy, t_old = [], [], []
        for _ in range(max(2, a.reps // 2)):
            t.invalidate()
            t_new.append(timed(lambda: eng.cluster_tri_nearest_host(t, K, KSPACE, MAX_D, -1.0))[0])
            t.invalidate()
            t_greedy.append(timed(lambda: eng.cluster_tri_greedy_host(t, K, KSPACE, MAX_D, -1.0))[0])
            t.invalidate()
            t_old.append(baseline(eng, t)[3])
        cell["per_table"] = summary(t_new, t_greedy, t_old)
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
