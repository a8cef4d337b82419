#!/usr/bin/env python3
"""Recorded stdout of the REFERENCE CLI for `mash dist -N` (tests/test_topk_gpu.py).

    make -C oracle refcli                      # oracle/_ref/mash-ref, from the reference's own unmodified sources
    python tests/golden/make_topk_golden.py    # writes tests/golden/topk/{family.fa.gz, outsiders.fa, *.out, cases.json}

The reference has no -N: what is recorded is its `mash dist` output, and tests/topk_model.py states what -N prints from it
(ranked by column 5 as an exact fraction).  The inputs: a seeded family of 40 related short sequences (four clades around one
root, two exact copies among them), sketched small (-i -k 16 -s 64) so that equal fractions abound, compared with itself.
A self-comparison can never leave a query without a line under -d (a sketch is at distance 0 from itself), so three unrelated
sequences (outsiders.fa) follow the family as further queries: they are the queries with no line under -d.

Conditions on the recording, asserted here (the seed is the first that meets them) and again by the test:
  * for every N in {1, 3, 10} some query of `dist` has a tie across the cut (its N-th and (N+1)-th best fractions are equal);
  * under -d some query has fewer than N lines for N = 3 and N = 10 (and at least one), and some query has none.
Never run by a test; only data is committed."""
import gzip, json, os, subprocess, sys, tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import topk_model as tm  # noqa: E402

OUT = os.path.join(HERE, "topk")
REFCLI = os.path.join(ROOT, "oracle", "_ref", "mash-ref")
SKETCH = ["-i", "-k", "16", "-s", "64"]
MAX_D, MAX_P = "0.08", "1e-10"
NS = (1, 3, 10)
COMMANDS = {"dist": [], "dist_d": ["-d", MAX_D], "dist_v": ["-v", MAX_P]}


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
    rng = np.random.default_rng(seed)
    root = rand_dna(rng, 2500)
    recs = []
    for c in range(4):
        clade = mutate(rng, root, 0.05)
        for m in range(10):
            seq = mutate(rng, clade, float(rng.choice([0.004, 0.01, 0.02, 0.04])))
            if m in (3, 7) and c < 2:
                seq = recs[-1][1]                                  # an exact copy of its neighbour
            recs.append((b"f%02d clade %d" % (len(recs), c), seq[: int(rng.integers(1500, 2500))] if m == 9 else seq))
    outsiders = [(b"o%d unrelated" % i, rand_dna(rng, 2000)) for i in range(3)]
    return recs, outsiders


def record(d, seed):
    recs, outsiders = family(seed)
    with gzip.GzipFile(f"{d}/family.fa.gz", "wb", mtime=0) as f:
        f.write(fasta(recs))
    open(f"{d}/outsiders.fa", "wb").write(fasta(outsiders))
    outs = {}
    for name, opts in COMMANDS.items():
        r = subprocess.run([REFCLI, "dist", *SKETCH, *opts, "family.fa.gz", "family.fa.gz", "outsiders.fa"], cwd=d, capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr[-300:]
        outs[name] = r.stdout.decode()
    return outs


def conditions(outs, nq):
    """(met, why not)"""
    for n in NS:
        if not tm.has_tie_across_cut(outs["dist"], n):
            return False, f"no tie across the cut at N = {n}"
    lines = [len(l) for _, l in tm.query_runs(outs["dist_d"])]
    for n in (3, 10):
        if not any(0 < x < n for x in lines):
            return False, f"-d: no query with fewer than {n} lines"
    if len(lines) >= nq:
        return False, "-d: no query without a line"
    if not any(x >= 10 for x in lines):
        return False, "-d: no query with 10 lines and more"
    if len(outs["dist_v"].splitlines()) in (0, len(outs["dist"].splitlines())):
        return False, "-v filters nothing or everything"
    return True, ""


def main():
    if not os.path.exists(REFCLI):
        sys.exit("build the reference CLI first: make -C oracle refcli")
    os.makedirs(OUT, exist_ok=True)
    for seed in range(20261017, 20261017 + 50):
        with tempfile.TemporaryDirectory(prefix="topkgold_") as d:
            outs = record(d, seed)
            ok, why = conditions(outs, 43)
            print(f"seed {seed}: {'ok' if ok else why}")
            if not ok:
                continue
            for f in ("family.fa.gz", "outsiders.fa"):
                open(f"{OUT}/{f}", "wb").write(open(f"{d}/{f}", "rb").read())
            for name, text in outs.items():
                open(f"{OUT}/{name}.out", "w").write(text)
                print(f"{name:8s} {len(text):8d} bytes")
            json.dump({"seed": seed, "queries": 43, "ns": list(NS), "inputs": ["family.fa.gz", "family.fa.gz", "outsiders.fa"],
                       "cases": [{"name": n, "cmd": ["dist", *SKETCH, *o]} for n, o in COMMANDS.items()]},
                      open(f"{OUT}/cases.json", "w"), indent=1)
            return
    sys.exit("no seed met the conditions")


if __name__ == "__main__":
    main()
