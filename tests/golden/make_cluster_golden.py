#!/usr/bin/env python3
"""Recorded stdout of the REFERENCE CLI for `mash cluster` (tests/test_cluster_model.py, tests/test_cluster_gpu.py).

    make -C oracle refcli                         # oracle/_ref/mash-ref, from the reference's own unmodified sources
    python tests/golden/make_cluster_golden.py    # writes tests/golden/cluster/{family.fa.gz, *.out, cases.json}

The reference has no cluster command: what is recorded is its `mash triangle -E` output under three -d values, one -v and one
-d with -v, and tests/cluster_model.py states what `mash cluster` prints from it (connected components of the printed pairs).
The input: a seeded family like make_topk_golden.py's -- four clades around one root, exact copies among them -- and a few
unrelated sequences, sketched small (-i -k 16 -s 64), the records SHUFFLED so that the clusters interleave in input order.

Conditions on the recording, asserted here (the seed is the first that meets them) and again by the test, on the recorded
text alone (cluster_model.fixture_conditions):
  (a) at some threshold a cluster that is not a clique;
  (b) in some case at least two singletons, a cluster of exactly two and one of ten or more;
  (c) a cluster whose members are not contiguous in input order, and one whose first edge in reference order joins two members
      neither of which is its smallest;
  (d) the three -d cases give three different partitions, and the -v case differs from no filter.
Never run by a test; only data is committed."""
import gzip, json, os, subprocess, sys, tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import cluster_model as cm  # noqa: E402

OUT = os.path.join(HERE, "cluster")
REFCLI = os.path.join(ROOT, "oracle", "_ref", "mash-ref")
SKETCH = ["-i", "-k", "16", "-s", "64"]
CASES = {"d1": ["-d", "0.01"], "d2": ["-d", "0.02"], "d3": ["-d", "0.05"], "v": ["-v", "1e-30"], "dv": ["-d", "0.11", "-v", "1e-37"]}


def rand_dna(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()


def mutate(rng, seq, rate):
    a = np.frombuffer(seq, dtype=np.uint8).copy()
    idx = np.nonzero(rng.random(len(a)) < rate)[0]
    a[idx] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, len(idx))]
    return a.tobytes()


def fasta(records, width=70):
    out = []
    for name, seq in records:
        out.append(b">" + name + b"\n")
        out += [seq[i:i + width] + b"\n" for i in range(0, len(seq), width)]
    return b"".join(out)


def family(seed):
    """(name, comment, sequence) in input order"""
    rng = np.random.default_rng(seed)
    root = rand_dna(rng, 2500)
    seqs = []
    for c in range(4):
        clade = mutate(rng, root, 0.05)
        for m in range(10):
            seq = mutate(rng, clade, float(rng.choice([0.004, 0.01, 0.02, 0.04])))
            if m in (3, 7) and c < 2:
                seq = seqs[-1][1]                                  # an exact copy of its neighbour
            seqs.append((c, seq[: int(rng.integers(1500, 2500))] if m == 9 else seq))
    seqs += [(9, rand_dna(rng, 2000)) for _ in range(4)]           # unrelated
    order = rng.permutation(len(seqs))
    return [("g%02d" % i, "member %02d of clade %d" % (i, seqs[j][0]), seqs[j][1]) for i, j in enumerate(order)]


def record(d, seed):
    recs = family(seed)
    with gzip.GzipFile(f"{d}/family.fa.gz", "wb", mtime=0) as f:
        f.write(fasta([((nm + " " + cmt).encode(), s) for nm, cmt, s in recs]))
    outs = {}
    for name, opts in CASES.items():
        r = subprocess.run([REFCLI, "triangle", "-E", *SKETCH, *opts, "family.fa.gz"], cwd=d, capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr[-300:]
        outs[name] = r.stdout.decode()
    return recs, outs


def main():
    if not os.path.exists(REFCLI):
        sys.exit("build the reference CLI first: make -C oracle refcli")
    os.makedirs(OUT, exist_ok=True)
    for seed in range(20261017, 20261017 + 200):
        with tempfile.TemporaryDirectory(prefix="clgold_") as d:
            recs, outs = record(d, seed)
            names = [r[0] for r in recs]
            ok, why = cm.fixture_conditions({k: cm.edges_of_stdout(t, names) for k, t in outs.items()}, len(names), "v")
            print(f"seed {seed}: {'ok' if ok else why}")
            if not ok:
                continue
            open(f"{OUT}/family.fa.gz", "wb").write(open(f"{d}/family.fa.gz", "rb").read())
            for name, text in outs.items():
                open(f"{OUT}/{name}.out", "w").write(text)
                e = cm.edges_of_stdout(text, names)
                lab = cm.labels(len(names), [x[0] for x in e], [x[1] for x in e])
                print(f"{name:3s} {len(text):7d} bytes, cluster sizes {sorted(len(m) for m in cm.clusters(lab).values())}, "
                      f"{len(cm.non_clique_clusters(lab, e))} not cliques")
            json.dump({"seed": seed, "input": "family.fa.gz", "sketch": SKETCH, "names": names, "comments": [r[1] for r in recs],
                       "cases": [{"name": n, "options": o} for n, o in CASES.items()]},
                      open(f"{OUT}/cases.json", "w"), indent=1)
            return
    sys.exit("no seed met the conditions")


if __name__ == "__main__":
    main()
