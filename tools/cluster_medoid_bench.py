#!/usr/bin/env python3
"""Single-linkage clusters with their medoids on the device (mg_cluster_tri_medoid_host, `mash cluster -M`) beside
  - mg_cluster_tri_host (`mash cluster`): the floor -- the same compare, ballots and unions, no score, no pick;
  - what a user does without it: mg_compare_tri_results_host (count first, then fetch the records, 32 bytes per edge) plus a
    numpy score-and-pick over the fetched records,
in one process on one device, at -d 0.05.

    python tools/cluster_medoid_bench.py [--reps 9] [--out profiles/cluster_medoid_bench.json]
    python tools/cluster_medoid_bench.py --only c3|species     # that table alone
    python tools/cluster_medoid_bench.py --variant aggregated|plain|both     # [both] the A/B of the union kernel
    python tools/cluster_medoid_bench.py --trace --only species              # the new call alone, --reps times per variant (for a kernel trace)

Tables: the C3 generator (100 000 sketches in clusters of 100, s = 1000) and one species of 32 768 sketches
(species_sketch_table).  Each is timed PER TABLE (a fresh table every repetition: the index build is inside the call) and as
FURTHER PASSES over a resident table.  Times are wall clock around calls that return finished host arrays; medians are reported.
Within a repetition the device calls follow the baseline, whose numpy part leaves the device idle for a few hundred milliseconds:
one untimed call of the floor stands between them, and the order of the timed calls rotates from one repetition to the next, so
that no variant always runs first.  label, medoid, score, the clusters and the edge count are compared with the numpy
result once per table and variant, BEFORE anything is timed.  Recorded beside the times: how many clusters have a medoid other
than their first member.  The two variants of the union kernel: `aggregated` combines the weights of a word's lanes that hold the
same row in the wave (one atomic per distinct row), `plain` (MASHGPU_MEDOID_PLAIN) sends two atomics per edge.  No target time: what
is measured is the extra over mg_cluster_tri_host in the same process (extra_over_floor_ms) and the ratio to the fetch-and-numpy
route (baseline_total_over_new)."""
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
    """connected components, labelled by their smallest row: pull both ends of every edge down, jump, until nothing moves"""
    lab = np.arange(n, dtype=np.int64)
    while True:
        m = np.minimum(lab[rows], lab[cols])
        new = lab.copy()
        for at in (rows, cols, lab[rows], lab[cols]):
            np.minimum.at(new, at, m)
        while True:
            j = new[new]
            if np.array_equal(j, new):
                break
            new = j
        if np.array_equal(new, lab):
            return lab
        lab = new


def host_medoid(n, rec):
    """labels, then per row the sum of its edges' weights floor(numer * 2^32 / max(denom, 1)), then per cluster the largest sum,
    ties to the smaller row -> label, medoid, score"""
    rows, cols = rec["row"].astype(np.int64), rec["col"].astype(np.int64)
    w = (rec["numer"].astype(np.uint64) << np.uint64(32)) // np.maximum(rec["denom"].astype(np.uint64), np.uint64(1))
    lab = host_labels(n, rows, cols)
    score = np.zeros(n, dtype=np.uint64)
    np.add.at(score, rows, w)
    np.add.at(score, cols, w)
    order = np.lexsort((np.arange(n), np.iinfo(np.uint64).max - score, lab))
    lead = np.ones(n, dtype=bool)
    lead[1:] = lab[order][1:] != lab[order][:-1]
    top = np.zeros(n, dtype=np.int64)
    top[lab[order][lead]] = order[lead]
    return lab.astype(np.uint32), top[lab].astype(np.uint32), score


def count_edges(eng, t):
    """mg_compare_tri_results_host with capacity 0: the count (MG_ERR_NOMEM is its way of saying so)"""
    import ctypes as C
    n = C.c_uint64(0)
    rc = eng.lib.mg_compare_tri_results_host(eng.ctx, t.handle, 0, t.rows, K, KSPACE, MAX_D, -1.0, None, 0, C.byref(n))
    assert rc in (abi.MG_OK, abi.MG_ERR_NOMEM), rc
    return int(n.value)


def baseline(eng, t):
    """-> label, medoid, score, edges, seconds of (the counting call, the fetching call alone, the numpy score-and-pick)"""
    t0 = time.perf_counter()
    n_edges = count_edges(eng, t)
    t1 = time.perf_counter()
    rec = eng.compare_tri_results(t, K, KSPACE, MAX_D, -1.0, capacity=max(n_edges, 1))
    t2 = time.perf_counter()
    lab, med, score = host_medoid(t.rows, rec)
    return lab, med, score, len(rec), (t1 - t0, t2 - t1, time.perf_counter() - t2)


def stats(v):
    return {"median_ms": 1e3 * statistics.median(v), "min_ms": 1e3 * min(v), "max_ms": 1e3 * max(v), "n": len(v)}


def summary(t_new, t_floor, t_old):
    """t_new: {variant: seconds per repetition}; t_old: (count, fetch, numpy) per repetition"""
    floor = statistics.median(t_floor)
    out = {"floor_cluster_tri": stats(t_floor), "baseline_count_call": stats([x[0] for x in t_old]),
           "baseline_results_alone": stats([x[1] for x in t_old]), "baseline_host_score_and_pick": stats([x[2] for x in t_old]),
           "baseline_total": stats([sum(x) for x in t_old])}
    for variant, v in t_new.items():
        new = statistics.median(v)
        out[variant] = {**stats(v), "extra_over_floor_ms": 1e3 * (new - floor), "new_over_floor": new / floor,
                        "new_over_results_alone": new / statistics.median([x[1] for x in t_old]),
                        "baseline_total_over_new": statistics.median([sum(x) for x in t_old]) / new}
    return out


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_medoid_bench.json"))
    ap.add_argument("--only", choices=["c3", "species"], default=None)
    ap.add_argument("--variant", choices=["aggregated", "plain", "both"], default="both")
    ap.add_argument("--trace", action="store_true", help="only the new call, --reps times per variant, nothing timed")
    a = ap.parse_args()
    torch.cuda.init()
    eng = MashGpu(0)
    variants = ["aggregated", "plain"] if a.variant == "both" else [a.variant]

    def medoid_call(t, variant, scores=False):
        eng.set_option("MASHGPU_MEDOID_PLAIN", "1" if variant == "plain" else None)
        try:
            return eng.cluster_tri_medoid_host(t, K, KSPACE, MAX_D, -1.0, scores=scores)
        finally:
            eng.set_option("MASHGPU_MEDOID_PLAIN", None)

    makers = {"c3": (100_000, lambda n: synth_torch.clustered_sketch_table(n, S, clusters=n // 100, device="cuda")),
              "species": (32_768, lambda n: synth_torch.species_sketch_table(n, S, device="cuda"))}
    res = {"device": torch.cuda.get_device_name(0), "sketch_size": S, "max_distance": MAX_D, "repetitions": a.reps, "variants": variants, "tables": []}
    for name, (n, make) in makers.items():
        if a.only and a.only != name:
            continue
        h, nh, ln = make(n)
        torch.cuda.synchronize()
        t = eng.table_wrap(h.data_ptr(), nh.data_ptr(), ln.data_ptr(), n, S)
        if a.trace:
            for variant in variants:
                for _ in range(a.reps):
                    medoid_call(t, variant)
            t.free()
            continue
        # outputs agree (and warm-up of all three) before anything is timed
        lab_old, med_old, score_old, ne_old, _ = baseline(eng, t)
        lab_floor, nc_floor, ne_floor = eng.cluster_tri_host(t, K, KSPACE, MAX_D, -1.0)
        for variant in variants:
            lab, med, score, nc, ne = medoid_call(t, variant, scores=True)
            assert ne == ne_old == ne_floor and nc == nc_floor, (name, variant, ne, ne_old, ne_floor, nc, nc_floor)
            assert np.array_equal(lab, lab_old) and np.array_equal(lab, lab_floor), (name, variant)
            assert np.array_equal(score, score_old), (name, variant, int((score != score_old).sum()))
            assert np.array_equal(med, med_old), (name, variant, int((med != med_old).sum()))
        roots = lab_old == np.arange(n)
        cell = {"table": name, "n": n, "edges": ne_old, "clusters": nc_floor, "outputs_equal_baseline": True,
                "clusters_with_a_medoid_other_than_their_first_member": int((med_old[roots] != np.arange(n)[roots]).sum()),
                "clusters_of_two_or_more": int((np.bincount(lab_old, minlength=n)[roots] >= 2).sum()),
                "baseline_record_bytes": ne_old * 32, "new_bytes": n * 8, "floor_bytes": n * 4}
        # further passes over the resident table
        t_new, t_floor, t_old = {v: [] for v in variants}, [], []
        legs = [*variants, "floor"]
        for r in range(a.reps):
            t_old.append(baseline(eng, t)[4])
            eng.cluster_tri_host(t, K, KSPACE, MAX_D, -1.0)                      # (untimed: the device has been idle behind numpy)
            for leg in legs[r % len(legs):] + legs[:r % len(legs)]:
                if leg == "floor":
                    t_floor.append(timed(lambda: eng.cluster_tri_host(t, K, KSPACE, MAX_D, -1.0))[0])
                else:
                    t_new[leg].append(timed(lambda: medoid_call(t, leg))[0])
        cell["further_passes"] = summary(t_new, t_floor, t_old)
        # per table: a fresh table each time, so the index build is inside the first call
        t_new, t_floor, t_old = {v: [] for v in variants}, [], []
        for r in range(max(len(legs), a.reps // 2)):
            t.invalidate()
            t_old.append(baseline(eng, t)[4])
            eng.cluster_tri_host(t, K, KSPACE, MAX_D, -1.0)
            for leg in legs[r % len(legs):] + legs[:r % len(legs)]:
                t.invalidate()
                if leg == "floor":
                    t_floor.append(timed(lambda: eng.cluster_tri_host(t, K, KSPACE, MAX_D, -1.0))[0])
                else:
                    t_new[leg].append(timed(lambda: medoid_call(t, leg))[0])
        cell["per_table"] = summary(t_new, t_floor, t_old)
        res["tables"].append(cell)
        print(json.dumps(cell), flush=True)
        t.free()
        del h, nh, ln
    if a.trace:
        return
    open(a.out, "w").write(json.dumps(res, indent=1) + "\n")
    print(json.dumps({"done": True, "tables": len(res["tables"])}))


if __name__ == "__main__":
    main()
