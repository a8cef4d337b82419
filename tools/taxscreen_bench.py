#!/usr/bin/env python3
"""Taxonomy of a screen at the bench's screen configuration: 100 000 synthetic sketches of s = 1000 (10^8 postings)
against a seeded random taxonomy of NCBI size.

    python tools/taxscreen_bench.py [--db 100000] [--nodes 2500000] [--reads 2000000] [--repeats 5] [--ref-rows 2000]

Times, each after a warm-up and over `--repeats` runs (wall clock around calls that end in a device synchronise):
  (a) mg_screen_set_taxa, once per database (the rows-by-hash index is built before, by a sparse finish), beside the
      reference: wall time of `oracle/_ref/mash-ref taxscreen -p 16` between its "Assigning LCA taxIDs" and "Writing
      output" messages on the first --ref-rows rows of the same database (0: skip; the reference rebuilds this for every run);
  (b) Screen.tax_finish per mixture beside Screen.finish_sparse of the same mixture, alternating.
Prints one JSON object."""
import argparse, json, os, statistics, subprocess, sys, tempfile, threading, time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from workloads import synth_torch  # noqa: E402
from mash_amd.abi import MashGpu, TAX_NONE  # noqa: E402

K, S, L, RL = 21, 1000, 1_000_000, 150


def random_taxonomy(n_nodes, n_rows, clusters, seed):
    """parent[i] uniform in [i / 2, i): depths around 50, NCBI's deepest lineages; rows of one cluster sit on nearby nodes, 2 % have none"""
    rng = np.random.default_rng(seed)
    i = np.arange(1, n_nodes)
    lo = i // 2
    parent = np.zeros(n_nodes, dtype=np.uint32)
    parent[1:] = lo + rng.integers(0, 1 << 40, n_nodes - 1) % (i - lo)
    base = rng.integers(0, n_nodes, max(clusters, 1))
    row_node = ((base[np.arange(n_rows) % max(clusters, 1)] + rng.integers(0, 64, n_rows)) % n_nodes).astype(np.uint32)
    row_node[rng.random(n_rows) < 0.02] = TAX_NONE
    return parent, row_node


def reference_lca_seconds(hashes, nhash, parent, row_node, rows):
    """the reference CLI on the first `rows` rows: seconds between its two stderr messages, or None"""
    ref, mash = os.path.join(ROOT, "oracle", "_ref", "mash-ref"), os.path.join(ROOT, "mash_amd", "bin", "mash")
    if not (os.path.exists(ref) and os.path.exists(mash)):
        return None
    with tempfile.TemporaryDirectory() as d:
        used = sorted({int(x) for x in row_node[:rows] if x != TAX_NONE})
        keep, stack = set(), list(used)
        while stack:                                   # the nodes the rows use and their ancestors; taxID = node + 1
            v = stack.pop()
            if v not in keep:
                keep.add(v)
                stack.append(int(parent[v]))
        with open(f"{d}/nodes.dmp", "w") as f, open(f"{d}/names.dmp", "w") as g:
            for v in sorted(keep):
                f.write(f"{v + 1}\t|\t{int(parent[v]) + 1}\t|\tno rank\t|\n")
                g.write(f"{v + 1}\t|\tnode {v}\t|\t\t|\tscientific name\t|\n")
        sk = [{"name": f"row{i}", "length": L, "comment": "" if row_node[i] == TAX_NONE else f"taxid {int(row_node[i]) + 1}",
               "hashes": [int(x) for x in hashes[i, : nhash[i]]]} for i in range(rows)]
        with open(f"{d}/db.json", "w") as f:             # the layout `mash info -d` prints, which `mash json2msh` reads back
            f.write('{\n "kmer" : %d,\n "alphabet" : "ACGT",\n "preserveCase" : false,\n "canonical" : true,\n "sketchSize" : %d,\n "hashType" : "MurmurHash3_x64_128",\n'
                    ' "hashBits" : 64,\n "hashSeed" : 42,\n "sketches" :\n [\n' % (K, S))
            for j, r in enumerate(sk):
                f.write('  {\n   "name" : "%s",\n   "length" : %d,\n   "comment" : "%s",\n   "hashes" :\n   [\n    %s\n   ]\n  }%s\n'
                        % (r["name"], r["length"], r["comment"], ",\n    ".join(map(str, r["hashes"])), "," if j + 1 < rows else ""))
            f.write(" ]\n}\n")
        if subprocess.run([mash, "json2msh", f"{d}/db.json", f"{d}/db.msh"], capture_output=True).returncode != 0:
            return None
        rng = np.random.default_rng(3)
        with open(f"{d}/pool.fa", "wb") as f:
            for i in range(200):
                f.write(b">r%d\n" % i + np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, RL)].tobytes() + b"\n")
        pr = subprocess.Popen([ref, "taxscreen", "-p", "16", "-t", d, f"{d}/db.msh", f"{d}/pool.fa"], stderr=subprocess.PIPE, stdout=subprocess.DEVNULL)
        t_begin = t_end = None
        killer = threading.Timer(240, pr.kill)           # (a database too large for the reference to finish: reported as unmeasured)
        killer.start()
        for line in pr.stderr:
            if line.startswith(b"Assigning LCA"):
                t_begin = time.perf_counter()
            elif line.startswith(b"Writing output"):
                t_end = time.perf_counter()
        pr.wait()
        killer.cancel()
        return None if pr.returncode != 0 or t_begin is None or t_end is None else t_end - t_begin


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--db", type=int, default=100_000)
    ap.add_argument("--src", type=int, default=1000, help="genomes the reads are sampled from")
    ap.add_argument("--nodes", type=int, default=2_500_000)
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ref-rows", type=int, default=2000)
    a = ap.parse_args()
    torch.cuda.init()
    eng = MashGpu(0)
    p = eng.params(k=K, s=S)
    genomes = synth_torch.synthetic_genomes(0, a.src, L, device="cuda", stride=40000)
    gh = torch.empty((a.src, S), dtype=torch.int64, device="cuda")
    gn = torch.empty(a.src, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.sketch_dev(genomes.data_ptr(), a.src * L, np.arange(a.src + 1, dtype=np.uint64) * np.uint64(L), p, gh.data_ptr(), gn.data_ptr())
    eng.synchronize()
    rest = max(0, a.db - a.src)
    clusters = max(1, rest // 100)
    fh, fn, _ = synth_torch.clustered_sketch_table(max(rest, 1), S, clusters=clusters, device="cuda")
    hashes = torch.cat([gh, fh[:rest]], 0).contiguous()
    nhash = torch.cat([gn, fn[:rest].to(torch.int32)], 0).contiguous()
    n = a.src + rest
    lengths = torch.full((n,), L, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    db = eng.table_wrap(hashes.data_ptr(), nhash.data_ptr(), lengths.data_ptr(), n, S)
    parent, row_node = random_taxonomy(a.nodes, n, clusters, seed=11)
    reads = synth_torch.synthetic_reads(genomes, a.reads, RL, seed=1000)
    torch.cuda.synchronize()
    res = {"device": torch.cuda.get_device_name(0), "db_sketches": n, "sketch_size": S, "taxonomy_nodes": a.nodes, "reads": a.reads, "repeats": a.repeats}
    tax = eng.taxonomy(parent)
    sc = eng.screen_open(db, p)
    sc.add_dev(reads.data_ptr(), int(reads.numel()))
    sc.finish_sparse()                                   # builds the rows-by-hash index (once per database, not timed here)

    def timed(fn):
        eng.synchronize()
        t0 = time.perf_counter()
        out = fn()
        eng.synchronize()
        return time.perf_counter() - t0, out

    # (a) once per database
    timed(lambda: sc.set_taxa(tax, row_node))
    t_set = [timed(lambda: sc.set_taxa(tax, row_node))[0] for _ in range(a.repeats)]
    res["set_taxa_s"] = {"median": statistics.median(t_set), "min": min(t_set), "max": max(t_set), "all": t_set}
    res["tax_note"] = sc.tax_note()
    # (b) per mixture, alternating with the sparse finish of the same mixture
    timed(sc.tax_finish)
    timed(sc.finish_sparse)
    t_tax, t_sparse = [], []
    for _ in range(a.repeats):
        dt, out = timed(sc.tax_finish)
        t_tax.append(dt)
        dt, hits = timed(sc.finish_sparse)
        t_sparse.append(dt)
    res["tax_finish_s"] = {"median": statistics.median(t_tax), "min": min(t_tax), "max": max(t_tax), "all": t_tax}
    res["finish_sparse_s"] = {"median": statistics.median(t_sparse), "min": min(t_sparse), "max": max(t_sparse), "all": t_sparse}
    res.update({"taxa_reported": int(len(out[0])), "observed_hashes": int(out[1]), "distinct_hashes": int(out[2]), "sparse_hits": int(len(hits[0]))})
    sc.close()
    tax.free()
    if a.ref_rows:
        rows = min(a.ref_rows, n)
        h = hashes[:rows].cpu().numpy().view(np.uint64)
        dt = reference_lca_seconds(h, nhash[:rows].cpu().numpy(), parent, row_node, rows)
        res["reference_lca"] = {"rows": rows, "postings": int(nhash[:rows].sum()), "threads": 16, "seconds": dt} if dt is not None else "unmeasured"
    print(json.dumps(res))


if __name__ == "__main__":
    main()
