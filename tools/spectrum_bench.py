#!/usr/bin/env python3
"""The distance spectrum on the device (mg_compare_tri_spectrum_host, `mash triangle -H`) beside what a user pays today, in one
process on one device:

  filters off   - mg_compare_tri_dev: the whole matrix of {numer, denom} written on the device and left there -- the floor before
                  anything is reduced (40 GB for 100 000 sketches);
                - mg_compare_tri_sparse_host (the pairs that share a hash, 16 bytes each to the host) plus a numpy `unique` and the
                  rule for every other pair;
  -d 0.05       - mg_compare_tri_results_host (count first, then fetch the records, 32 bytes each) plus a numpy `unique`;
  identical rows- the combining kernel beside the plain one (MASHGPU_SPECTRUM_PLAIN): every pair falls into the bin s/s.

    python tools/spectrum_bench.py [--reps 5] [--out profiles/spectrum_bench.json]
    python tools/spectrum_bench.py --only c3|species     # that table alone (the identical rows go with `species`)

Tables: the C3 generator (100 000 sketches in clusters of 100, s = 1000) and one species of 32 768 sketches (species_sketch_table);
16 384 copies of one sketch for the hot bin.  Each is timed PER TABLE (mg_table_invalidate before every call: the index build is
inside it) and as FURTHER PASSES over a resident table.  Times are wall clock around calls that return finished host arrays (the
floor: around the call and a stream synchronisation); medians are reported, with the route the spectrum call took and its stats.
Equality with the numpy result is asserted once per table and filter BEFORE anything is timed.  Where the pairs that share a hash
are more than 2^27 (one species, filters off: nearly all of them -- 16 bytes each would be gigabytes to fetch and sort) that baseline
is not run and the judge is a torch.unique over the floor's matrix on the device.  No target time: what is recorded is the ratio to the floor and to the baselines."""
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


def unique_bins(numer, denom):
    """{(numer, denom): pairs} of two arrays"""
    keys, counts = np.unique(numer.astype(np.uint64) << np.uint64(32) | denom.astype(np.uint64), return_counts=True)
    return {(int(k) >> 32, int(k) & 0xFFFFFFFF): int(c) for k, c in zip(keys, counts)}


def rule_bins(nhash, s):
    """{D: pairs} of the whole triangle if no pair shared a hash: D = min(s, |A| + |B|), |X| = min(nhash, s)"""
    sizes, h = np.unique(np.minimum(nhash.astype(np.int64), s), return_counts=True)
    out = {}
    for a in range(len(sizes)):
        for b in range(a, len(sizes)):
            n = int(h[a]) * (int(h[a]) - 1) // 2 if a == b else int(h[a]) * int(h[b])
            d = min(s, int(sizes[a] + sizes[b]))
            if n:
                out[d] = out.get(d, 0) + n
    return out


def count_sparse(eng, t):
    """mg_compare_tri_sparse_host with capacity 0: the count (MG_ERR_NOMEM is its way of saying so)"""
    n = C.c_uint64(0)
    rc = eng.lib.mg_compare_tri_sparse_host(eng.ctx, t.handle, 0, t.rows, None, 0, C.byref(n))
    assert rc in (abi.MG_OK, abi.MG_ERR_NOMEM), rc
    return int(n.value)


def baseline_sparse(eng, t, nhash):
    """filters off without the spectrum call: the exceptions, a numpy unique, the rule -> bins, seconds of (device call, numpy)"""
    t0 = time.perf_counter()
    edges = eng.compare_tri_sparse(t, capacity=max(count_sparse(eng, t), 1))
    t1 = time.perf_counter()
    bins = unique_bins(edges["numer"], edges["denom"])
    rule = rule_bins(nhash, S)
    ca, cb = np.minimum(nhash[edges["row"]].astype(np.int64), S), np.minimum(nhash[edges["col"]].astype(np.int64), S)
    for d, c in zip(*np.unique(np.minimum(ca + cb, S), return_counts=True)):
        rule[int(d)] -= int(c)
    for d, c in rule.items():
        if c:
            bins[(0, d)] = bins.get((0, d), 0) + c
    return bins, len(edges), (t1 - t0, time.perf_counter() - t1)


def baseline_results(eng, t):
    """-d 0.05 without the spectrum call: count, fetch, numpy unique -> bins, records, seconds of (count, fetch, numpy)"""
    t0 = time.perf_counter()
    n = C.c_uint64(0)
    rc = eng.lib.mg_compare_tri_results_host(eng.ctx, t.handle, 0, t.rows, K, KSPACE, MAX_D, -1.0, None, 0, C.byref(n))
    assert rc in (abi.MG_OK, abi.MG_ERR_NOMEM), rc
    t1 = time.perf_counter()
    rec = eng.compare_tri_results(t, K, KSPACE, MAX_D, -1.0, capacity=max(int(n.value), 1))
    t2 = time.perf_counter()
    return unique_bins(rec["numer"], rec["denom"]), len(rec), (t1 - t0, t2 - t1, time.perf_counter() - t2)


def as_dict(bins):
    return {(int(x["numer"]), int(x["denom"])): int(x["count"]) for x in bins}


def in_order(bins):
    frac = [(int(x["numer"]) if x["denom"] else 1, int(x["denom"]) if x["denom"] else 1, int(x["denom"])) for x in bins]
    return all(a[0] * b[1] > b[0] * a[1] or (a[0] * b[1] == b[0] * a[1] and a[2] < b[2]) for a, b in zip(frac, frac[1:]))


def stats(v):
    return {"median_ms": 1e3 * statistics.median(v), "min_ms": 1e3 * min(v), "max_ms": 1e3 * max(v), "n": len(v)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectrum_bench.json"))
    ap.add_argument("--only", choices=["c3", "species"], default=None)
    a = ap.parse_args()
    torch.cuda.init()
    eng = MashGpu(0)

    def spectrum(t, max_d=-1.0, plain=False):
        eng.set_option("MASHGPU_SPECTRUM_PLAIN", "1" if plain else None)
        try:
            return eng.tri_spectrum(t, K, KSPACE, max_d, -1.0)
        finally:
            eng.set_option("MASHGPU_SPECTRUM_PLAIN", None)

    def passes(t, legs, fresh):
        """{leg: seconds per repetition}; fresh: the table's derived data is dropped before every call"""
        out = {name: [] for name in legs}
        names = list(legs)
        for r in range(a.reps):
            for name in names[r % len(names):] + names[:r % len(names)]:
                reps_of_leg = legs[name][1]
                if len(out[name]) >= reps_of_leg:
                    continue
                if fresh:
                    t.invalidate()
                out[name].append(timed(legs[name][0])[0])
        return out

    makers = {"c3": (100_000, lambda n: synth_torch.clustered_sketch_table(n, S, clusters=n // 100, device="cuda")),
              "species": (32_768, lambda n: synth_torch.species_sketch_table(n, S, device="cuda"))}
    res = {"device": torch.cuda.get_device_name(0), "sketch_size": S, "max_distance": MAX_D, "repetitions": a.reps, "tables": []}
    for name, (n, make) in makers.items():
        if a.only and a.only != name:
            continue
        h, nh, ln = make(n)
        torch.cuda.synchronize()
        nhash = nh.cpu().numpy()
        t = eng.table_wrap(h.data_ptr(), nh.data_ptr(), ln.data_ptr(), n, S)
        pairs = n * (n - 1) // 2
        matrix = torch.empty((pairs, 2), dtype=torch.int32, device="cuda")        # the floor's output: 8 bytes per pair, left on the device

        def floor():
            eng.compare_tri_dev(t, 0, n, matrix.data_ptr())
            eng.synchronize()

        # equality first (and warm-up of every leg)
        shared_pairs = count_sparse(eng, t)
        heavy = shared_pairs > (1 << 27)
        if heavy:
            floor()
            keys, counts = torch.unique(matrix.view(torch.int64).flatten(), return_counts=True)      # (numer in the low word, denom in the high one)
            want_off = {(int(k) & 0xFFFFFFFF, int(k) >> 32): int(c) for k, c in zip(keys.cpu().numpy(), counts.cpu().numpy())}
            del keys, counts
        else:
            want_off = baseline_sparse(eng, t, nhash)[0]
        got = spectrum(t)
        st_off = eng.spectrum_stats()
        assert as_dict(got) == want_off and in_order(got) and sum(want_off.values()) == pairs, (name, "filters off", len(got), len(want_off))
        assert as_dict(spectrum(t, plain=True)) == want_off
        want_d, records, _ = baseline_results(eng, t)
        got_d = spectrum(t, MAX_D)
        st_d = eng.spectrum_stats()
        assert as_dict(got_d) == want_d and in_order(got_d), (name, "-d", len(got_d), len(want_d))
        floor()
        cell = {"table": name, "n": n, "pairs": pairs, "equal_to_numpy": True,
                "filters_off": {"bins": len(got), "pairs_that_share_a_hash": shared_pairs, "stats": st_off, "spectrum_bytes": 16 * len(got),
                                "matrix_bytes": 8 * pairs, "sparse_bytes": 16 * shared_pairs},
                "d_0.05": {"bins": len(got_d), "passing_pairs": records, "stats": st_d, "spectrum_bytes": 16 * len(got_d), "record_bytes": 32 * records}}
        for fresh, key in ((False, "further_passes"), (True, "per_table")):
            legs = {"spectrum": (lambda: spectrum(t), a.reps), "matrix_on_device": (floor, a.reps)}
            if not heavy:
                legs["sparse_and_numpy"] = (lambda: baseline_sparse(eng, t, nhash), a.reps)
            got_t = passes(t, legs, fresh)
            sp, fl = statistics.median(got_t["spectrum"]), statistics.median(got_t["matrix_on_device"])
            cell["filters_off"][key] = {**{k: stats(v) for k, v in got_t.items()}, "spectrum_over_matrix_on_device": sp / fl,
                                        "sparse_and_numpy_over_spectrum": None if heavy else statistics.median(got_t["sparse_and_numpy"]) / sp}
            got_t = passes(t, {"spectrum": (lambda: spectrum(t, MAX_D), a.reps), "results_and_numpy": (lambda: baseline_results(eng, t), a.reps)}, fresh)
            sp, ba = (statistics.median(got_t[k]) for k in ("spectrum", "results_and_numpy"))
            cell["d_0.05"][key] = {**{k: stats(v) for k, v in got_t.items()}, "results_and_numpy_over_spectrum": ba / sp}
        res["tables"].append(cell)
        print(json.dumps(cell), flush=True)
        t.free()
        del matrix, h, nh, ln
        torch.cuda.empty_cache()
    if a.only in (None, "species"):
        # every pair in s/s: the combining kernel beside the plain one
        n = 16_384
        h, nh, ln = synth_torch.identical_sketch_table(n, S, device="cuda")
        torch.cuda.synchronize()
        t = eng.table_wrap(h.data_ptr(), nh.data_ptr(), ln.data_ptr(), n, S)
        pairs = n * (n - 1) // 2
        cell = {"table": "identical", "n": n, "pairs": pairs}
        for label, max_d in (("filters_off", -1.0), ("d_0.05", MAX_D)):
            for plain in (False, True):
                got = spectrum(t, max_d, plain)
                assert as_dict(got) == {(S, S): pairs}, (label, plain, as_dict(got))
            st = eng.spectrum_stats()
            got_t = passes(t, {"combining": (lambda: spectrum(t, max_d), a.reps), "plain": (lambda: spectrum(t, max_d, True), a.reps)}, False)
            cell[label] = {"stats": st, **{k: stats(v) for k, v in got_t.items()},
                           "plain_over_combining": statistics.median(got_t["plain"]) / statistics.median(got_t["combining"])}
        res["tables"].append(cell)
        print(json.dumps(cell), flush=True)
        t.free()
    open(a.out, "w").write(json.dumps(res, indent=1) + "\n")
    print(json.dumps({"done": True, "tables": len(res["tables"])}))


if __name__ == "__main__":
    main()
