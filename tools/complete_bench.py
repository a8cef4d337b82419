#!/usr/bin/env python3
"""Complete-linkage clusters on the device (mg_cluster_tri_complete_host) beside two neighbours of the same run, in one process on
one device, at -d 0.05:
  * mg_cluster_tri_host alone -- the FLOOR: the same compare and ballots, no edge list, no index, no rounds;
  * mg_compare_tri_results_host, count first, then fetch the records (32 bytes per edge) -- what a host implementation of complete
    linkage must pay BEFORE it starts (its O(n^2) algorithm is not timed here: tests/complete_model.py is no contender).

    python tools/complete_bench.py [--reps 5] [--model-seconds 60] [--out profiles/complete_bench.json]
    python tools/complete_bench.py --only c3|species     # the new call alone, --reps times (for a kernel trace)

Tables: the C3 generator (100 000 sketches in clusters of 100, s = 1000) and one species of 32 768 sketches
(species_sketch_table).  Each is timed PER TABLE (a fresh table every repetition: the index build is inside the call) and as FURTHER
PASSES over a resident table.  Times are wall clock around calls that return finished host arrays; the calls alternate within a
repetition; medians are reported.  Before anything is timed the labels are compared with tests/complete_model.py (walk_fast over the
records of mg_compare_tri_results_host) on a PREFIX of the table's rows: the prefix doubles from 2 048 rows while the model is
expected to finish within --model-seconds; its size and the model's time are recorded.  On the whole table the partition is checked
for what needs no model: every cluster a clique of the fetched records, label[i] <= i, labels idempotent.  No time is a condition.
Recorded beside the times: rounds, batches, regrows, and per round the links alive when it began and the links it merged
(mg_cluster_complete_rounds)."""
import argparse, json, os, statistics, sys, time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from workloads import synth_torch  # noqa: E402
from mash_amd import abi  # noqa: E402
from mash_amd.abi import MashGpu  # noqa: E402
from tests import complete_model  # noqa: E402

K, S = 21, 1000
KSPACE = 4.0 ** K
MAX_D = 0.05


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


def summary(t_new, t_single, t_old):
    new = statistics.median(t_new)
    return {"new": stats(t_new), "single_linkage": stats(t_single), "results_count_call": stats([x[0] for x in t_old]),
            "results_fetch_alone": stats([x[1] for x in t_old]), "results_count_and_fetch": stats([sum(x) for x in t_old]),
            "new_over_single_linkage": new / statistics.median(t_single),
            "new_over_results_count_and_fetch": new / statistics.median([sum(x) for x in t_old])}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def cliques(label, rec):
    """every cluster is a clique of the records: a cluster of k rows holds k (k - 1) / 2 of them, and a record is counted once"""
    inside = label[rec["row"]] == label[rec["col"]]
    have = np.bincount(label[rec["row"][inside]], minlength=len(label))
    size = np.bincount(label, minlength=len(label)).astype(np.int64)
    return bool(np.array_equal(have, size * (size - 1) // 2))


def model_prefix(eng, ptrs, n, budget):
    """the labels against the model on the largest prefix of the rows it is expected to finish within `budget` seconds"""
    p, done = min(2048, n), None
    while True:
        t = eng.table_wrap(*ptrs, p, S)
        label, nc, ne = eng.cluster_tri_complete_host(t, K, KSPACE, MAX_D, -1.0)
        rec, _ = fetch(eng, t)
        t.free()
        secs, want = timed(lambda: complete_model.walk_fast(p, rec["row"], rec["col"], rec["numer"], rec["denom"]))
        assert ne == len(rec) and np.array_equal(label, np.array(want, dtype=np.uint32)) and nc == len(set(want)), ("prefix", p, ne, len(rec))
        done = {"rows": p, "edges": ne, "clusters": nc, "model_seconds": secs, "labels_equal_model": True}
        if p == n or 4.5 * secs > budget:                      # (the rows double: about four times the edges)
            return done
        p = min(2 * p, n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--model-seconds", type=float, default=60.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=["c3", "species"], default=None)
    a = ap.parse_args()
    torch.cuda.init()
    eng = MashGpu(0)
    makers = {"c3": (100_000, lambda n: synth_torch.clustered_sketch_table(n, S, clusters=n // 100, device="cuda")),
              "species": (32_768, lambda n: synth_torch.species_sketch_table(n, S, device="cuda"))}
    res = {"device": torch.cuda.get_device_name(0), "sketch_size": S, "max_distance": MAX_D, "repetitions": a.reps, "tables": []}
    complete = lambda t: eng.cluster_tri_complete_host(t, K, KSPACE, MAX_D, -1.0)  # noqa: E731
    single = lambda t: eng.cluster_tri_host(t, K, KSPACE, MAX_D, -1.0)             # noqa: E731
    for name, (n, make) in makers.items():
        if a.only and a.only != name:
            continue
        h, nh, ln = make(n)
        torch.cuda.synchronize()
        ptrs = (h.data_ptr(), nh.data_ptr(), ln.data_ptr())
        t = eng.table_wrap(*ptrs, n, S)
        if a.only:
            for _ in range(a.reps + 2):
                complete(t)
            return
        side = MashGpu(0)                                      # (a context of its own: the timed one has seen the whole table only)
        prefix = model_prefix(side, ptrs, n, a.model_seconds)
        side.close()
        # the whole table: what needs no model (and the warm-up of all three)
        label, nc, ne = complete(t)
        st = eng.cluster_complete_stats()
        live, merged = eng.cluster_complete_rounds()
        rec, _ = fetch(eng, t)
        lab_single, nc_single, ne_single = single(t)
        lab = label.astype(np.int64)
        assert ne == len(rec) == ne_single and nc >= nc_single and nc == int((lab == np.arange(n)).sum()), (name, ne, len(rec), ne_single)
        assert np.all(lab <= np.arange(n)) and np.array_equal(lab[lab], lab) and np.array_equal(lab_single[lab], lab_single) and cliques(lab, rec), name
        assert live[0] == ne and live[-1] == 0 and sum(merged) == n - nc, name
        del rec
        slots = 2 * ne + 1
        cell = {"table": name, "n": n, "edges": ne, "clusters": nc, "single_linkage_clusters": nc_single, "model_prefix": prefix,
                "every_cluster_a_clique": True, "rounds": st["rounds"], "batches": st["batches"], "regrows": st["regrows"],
                "edge_capacity": st["edge_capacity"], "live_links_per_round": live, "merged_per_round": merged,
                "results_record_bytes": ne * 32, "new_bytes": n * 4, "device_bytes": st["edge_capacity"] * 16 + ne * 16 + slots * 16}
        # further passes over the resident table
        t_new, t_single, t_old = [], [], []
        for _ in range(a.reps):
            t_new.append(timed(lambda: complete(t))[0])
            t_old.append(fetch(eng, t)[1])
            t_single.append(timed(lambda: single(t))[0])
        cell["further_passes"] = summary(t_new, t_single, t_old)
        # per table: a fresh table each time, so the index build is inside the first call
        t_new, t_single, t_old = [], [], []
        for _ in range(a.reps):
            t.invalidate()
            t_new.append(timed(lambda: complete(t))[0])
            t.invalidate()
            t_old.append(fetch(eng, t)[1])
            t.invalidate()
            t_single.append(timed(lambda: single(t))[0])
        cell["per_table"] = summary(t_new, t_single, t_old)
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
