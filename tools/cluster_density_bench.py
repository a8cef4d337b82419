#!/usr/bin/env python3
"""Density clusters on the device (mg_cluster_tri_density_host, `mash cluster -D`) beside
  - mg_cluster_tri_nearest_host (`mash cluster -B`): the floor -- the same compare, ballots and 16-byte edge list, with the greedy
    rounds and two passes over the list behind it where the density call has six;
  - what a user pays today: mg_compare_tri_results_host (count first, then fetch the records, 32 bytes per edge) plus the
    definition over the fetched records in numpy (degrees by bincount, the core components by label propagation, the borders by a
    sort on the 64-bit key of forest_key.h),
in one process on one device, at -d 0.05.

    python tools/cluster_density_bench.py [--reps 5] [--out profiles/cluster_density_bench.json]
    python tools/cluster_density_bench.py --only c3|species     # the new call alone, --reps times (for a kernel trace)

Tables: the C3 generator (100 000 sketches in clusters of 100, s = 1000) and one species of 32 768 sketches
(species_sketch_table).  m is the median of the table's measured degrees (at least 1); the degree quantiles are recorded beside it.
Each table is timed PER TABLE (a fresh table every repetition: the index build is inside the call) and as FURTHER PASSES over a
resident table, medians of --reps.  Times are wall clock around calls that return finished host arrays; the calls alternate within
a repetition.  label, via, degree, the clusters and the edge count are compared with the numpy model once per table, BEFORE
anything is timed.  The degree pass is timed in both forms (MASHGPU_DENSITY_PLAIN).  The numpy model is timed in the further
passes only; the per-table baseline adds that median to its own count and fetch.  No target time: what is recorded is the call's
time, its excess over the floor, and whether it beats fetch-and-numpy."""
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
QUANTILES = (0, 10, 25, 50, 75, 90, 100)


def components(n, rows, cols):
    """label[i] = the smallest row of i's component under the edges {rows, cols}: labels pulled down edge by edge, then jumped"""
    lab = np.arange(n, dtype=np.int64)
    while True:
        m = np.minimum(lab[rows], lab[cols])
        new = lab.copy()
        np.minimum.at(new, rows, m)
        np.minimum.at(new, cols, m)
        np.minimum.at(new, lab[rows], m)
        np.minimum.at(new, lab[cols], m)
        while True:
            j = new[new]
            if np.array_equal(j, new):
                break
            new = j
        if np.array_equal(new, lab):
            return lab
        lab = new


def degrees(n, rec):
    return np.bincount(rec["row"], minlength=n) + np.bincount(rec["col"], minlength=n)


def host_density(n, rec, m):
    """the definition over fetched records -> label, via, degree"""
    rows, cols = rec["row"].astype(np.int64), rec["col"].astype(np.int64)
    deg = np.bincount(rows, minlength=n) + np.bincount(cols, minlength=n)
    core = deg >= m
    both = core[rows] & core[cols]
    lab = components(n, rows[both], cols[both])
    one = core[rows] != core[cols]
    r1, c1 = rows[one], cols[one]
    member = np.where(core[r1], c1, r1)
    centre = np.where(core[r1], r1, c1)
    key = (rec["numer"][one].astype(np.uint64) << np.uint64(42)) // np.maximum(rec["denom"][one].astype(np.uint64), np.uint64(1))
    order = np.lexsort((centre, np.iinfo(np.uint64).max - key, member))
    member, centre = member[order], centre[order]
    lead = np.ones(len(member), dtype=bool)
    lead[1:] = member[1:] != member[:-1]
    via = np.arange(n, dtype=np.int64)
    via[member[lead]] = centre[lead]
    root = lab[via]
    first = np.full(n, n, dtype=np.int64)
    np.minimum.at(first, root, np.arange(n, dtype=np.int64))
    return first[root].astype(np.uint32), via.astype(np.uint32), deg.astype(np.uint32)


def count_edges(eng, t):
    """mg_compare_tri_results_host with capacity 0: the count (MG_ERR_NOMEM is its way of saying so)"""
    import ctypes as C
    n = C.c_uint64(0)
    rc = eng.lib.mg_compare_tri_results_host(eng.ctx, t.handle, 0, t.rows, K, KSPACE, MAX_D, -1.0, None, 0, C.byref(n))
    assert rc in (abi.MG_OK, abi.MG_ERR_NOMEM), rc
    return int(n.value)


def fetch(eng, t):
    """-> records, seconds of (the counting call, the fetching call alone)"""
    t0 = time.perf_counter()
    n_edges = count_edges(eng, t)
    t1 = time.perf_counter()
    rec = eng.compare_tri_results(t, K, KSPACE, MAX_D, -1.0, capacity=max(n_edges, 1))
    return rec, (t1 - t0, time.perf_counter() - t1)


def stats(v):
    return {"median_ms": 1e3 * statistics.median(v), "min_ms": 1e3 * min(v), "max_ms": 1e3 * max(v), "n": len(v)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def summary(t_new, t_plain, t_floor, t_fetch, numpy_s):
    """t_fetch: (count, fetch) per repetition; numpy_s: the model's median seconds"""
    new, floor = statistics.median(t_new), statistics.median(t_floor)
    total = statistics.median([sum(x) for x in t_fetch]) + numpy_s
    return {"new": stats(t_new), "new_plain_degrees": stats(t_plain), "floor_nearest": stats(t_floor),
            "baseline_count_call": stats([x[0] for x in t_fetch]), "baseline_results_alone": stats([x[1] for x in t_fetch]),
            "baseline_numpy_model_ms": 1e3 * numpy_s, "baseline_total_ms": 1e3 * total,
            "excess_over_floor_ms": 1e3 * (new - floor), "new_over_floor": new / floor,
            "plain_minus_combined_ms": 1e3 * (statistics.median(t_plain) - new),
            "baseline_total_over_new": total / new, "beats_fetch_and_numpy": bool(new < total)}


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

    def new_call(t, m, plain=False):
        eng.set_option("MASHGPU_DENSITY_PLAIN", "1" if plain else None)
        try:
            return eng.cluster_tri_density_host(t, K, KSPACE, m, MAX_D, -1.0)
        finally:
            eng.set_option("MASHGPU_DENSITY_PLAIN", None)

    for name, (n, make) in makers.items():
        if a.only and a.only != name:
            continue
        h, nh, ln = make(n)
        torch.cuda.synchronize()
        t = eng.table_wrap(h.data_ptr(), nh.data_ptr(), ln.data_ptr(), n, S)
        # the degree distribution picks m; outputs agree (and warm-up of all three) before anything is timed
        rec, _ = fetch(eng, t)
        q = np.percentile(degrees(n, rec), QUANTILES, method="lower").astype(np.int64)
        m = max(1, int(q[QUANTILES.index(50)]))
        if a.only:
            for _ in range(a.reps + 2):
                new_call(t, m)
            return
        label, via, deg, nc, ne = new_call(t, m)
        st = eng.cluster_density_stats()
        w_label, w_via, w_deg = host_density(n, rec, m)
        assert ne == len(rec) and np.array_equal(deg, w_deg) and np.array_equal(via, w_via) and np.array_equal(label, w_label), \
            (name, ne, len(rec), int((deg != w_deg).sum()), int((via != w_via).sum()), int((label != w_label).sum()))
        assert nc == int((w_label == np.arange(n)).sum())
        p_label, p_via, p_deg, p_nc, p_ne = new_call(t, m, plain=True)
        assert np.array_equal(p_label, label) and np.array_equal(p_via, via) and np.array_equal(p_deg, deg) and (p_nc, p_ne) == (nc, ne)
        _, nc_floor, ne_floor = eng.cluster_tri_nearest_host(t, K, KSPACE, MAX_D, -1.0)
        assert ne_floor == ne
        _, nc_single, _ = eng.cluster_tri_host(t, K, KSPACE, MAX_D, -1.0)
        cell = {"table": name, "n": n, "edges": ne, "min_neighbours": m, "degree_quantiles": dict(zip(map(str, QUANTILES), map(int, q))),
                "clusters": nc, "cores": st["cores"], "borders": st["borders"], "noise": st["noise"], "single_linkage_clusters": nc_single,
                "regrows": st["regrows"], "edge_capacity": st["edge_capacity"], "outputs_equal_numpy_model": True,
                "borders_first_in_their_cluster": int(((deg < m) & (via != np.arange(n)) & (label == np.arange(n))).sum()),
                "list_bytes": ne * 16, "baseline_record_bytes": ne * 32, "new_bytes": n * 12}
        # further passes over the resident table
        t_new, t_plain, t_floor, t_fetch, t_numpy = [], [], [], [], []
        for _ in range(a.reps):
            t_new.append(timed(lambda: new_call(t, m))[0])
            t_plain.append(timed(lambda: new_call(t, m, plain=True))[0])
            t_floor.append(timed(lambda: eng.cluster_tri_nearest_host(t, K, KSPACE, MAX_D, -1.0))[0])
            rec, tf = fetch(eng, t)
            t_fetch.append(tf)
            t_numpy.append(timed(lambda: host_density(n, rec, m))[0])
        numpy_s = statistics.median(t_numpy)
        cell["further_passes"] = summary(t_new, t_plain, t_floor, t_fetch, numpy_s)
        cell["further_passes"]["baseline_numpy_model"] = stats(t_numpy)
        # per table: a fresh table each time, so the index build is inside the first call
        t_new, t_plain, t_floor, t_fetch = [], [], [], []
        for _ in range(a.reps):
            t.invalidate()
            t_new.append(timed(lambda: new_call(t, m))[0])
            t.invalidate()
            t_plain.append(timed(lambda: new_call(t, m, plain=True))[0])
            t.invalidate()
            t_floor.append(timed(lambda: eng.cluster_tri_nearest_host(t, K, KSPACE, MAX_D, -1.0))[0])
            t.invalidate()
            t_fetch.append(fetch(eng, t)[1])
        cell["per_table"] = summary(t_new, t_plain, t_floor, t_fetch, numpy_s)
        res["tables"].append(cell)
        print(json.dumps(cell), flush=True)
        t.free()
        del h, nh, ln, rec
    text = json.dumps(res, indent=1)
    if a.out:
        open(a.out, "w").write(text + "\n")
    print(json.dumps({"done": True, "tables": len(res["tables"])}))


if __name__ == "__main__":
    main()
