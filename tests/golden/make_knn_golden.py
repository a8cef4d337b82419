#!/usr/bin/env python3
"""Recorded stdout of the REFERENCE CLI for `mash triangle -N` (tests/test_knn_model.py, tests/test_knn_gpu.py).

    make -C oracle refcli                     # oracle/_ref/mash-ref, from the reference's own unmodified sources
    python tests/golden/make_knn_golden.py    # writes tests/golden/knn/{triangle*.out, cases.json}

The reference has no -N: what is recorded is its `mash triangle -E` output, and tests/knn_model.py states what -N prints from
it.  The inputs are those of tests/golden/topk, read in place (family.fa.gz outsiders.fa: 43 sketches, -i -k 16 -s 64 -- a
seeded family with two exact copies among its members, and three unrelated sequences).

Conditions on the recording, asserted here and again by tests/test_knn_model.py:
  * for every N in {1, 3, 10} some row of the unfiltered recording has a tie across the cut;
  * some row has a tie whose two neighbours lie on opposite sides of the diagonal;
  * under -d some row has no line, some has fewer than 3, some fewer than 10, some 10 and more;
  * -v filters something and not everything.
Never run by a test; only data is committed."""
import json, os, subprocess, sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import knn_model as km  # noqa: E402

OUT = os.path.join(HERE, "knn")
IN = os.path.join(HERE, "topk")
REFCLI = os.path.join(ROOT, "oracle", "_ref", "mash-ref")
SKETCH = ["-i", "-k", "16", "-s", "64"]
INPUTS = ["family.fa.gz", "outsiders.fa"]
MAX_D, MAX_P = "0.08", "1e-10"
NS = (1, 3, 10)
COMMANDS = {"triangle": ["-E"], "triangle_d": ["-E", "-d", MAX_D], "triangle_v": ["-E", "-v", MAX_P]}


def names_of(plain):
    """the sketches in input order: row i of a triangle first appears in column 1 (row 0 only as the second name of row 1's line)"""
    names = []
    for ln in plain.splitlines():
        a, b = ln.split("\t")[:2]
        if not names:
            names.append(b)
        if a != names[-1]:
            names.append(a)
    return names


def conditions(outs, names):
    """(met, why not)"""
    for n in NS:
        if not km.has_tie_across_cut(outs["triangle"], names, n):
            return False, f"no tie across the cut at N = {n}"
    if not km.has_tie_across_diagonal(outs["triangle"], names):
        return False, "no tie across the diagonal"
    lines = [len(r) for r in km.entries_of_stdout(outs["triangle_d"], names)]
    for what, ok in (("without a line", any(x == 0 for x in lines)), ("with fewer than 3 lines", any(0 < x < 3 for x in lines)),
                     ("with fewer than 10 lines", any(3 <= x < 10 for x in lines)), ("with 10 lines and more", any(x >= 10 for x in lines))):
        if not ok:
            return False, f"-d: no row {what}"
    if len(outs["triangle_v"].splitlines()) in (0, len(outs["triangle"].splitlines())):
        return False, "-v filters nothing or everything"
    return True, ""


def main():
    if not os.path.exists(REFCLI):
        sys.exit("build the reference CLI first: make -C oracle refcli")
    outs = {}
    for name, opts in COMMANDS.items():
        r = subprocess.run([REFCLI, "triangle", *SKETCH, *opts, *INPUTS], cwd=IN, capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr[-300:]
        outs[name] = r.stdout.decode()
    names = names_of(outs["triangle"])
    ok, why = conditions(outs, names)
    if not ok:
        sys.exit("the inputs of tests/golden/topk do not meet the conditions: " + why)
    os.makedirs(OUT, exist_ok=True)
    for name, text in outs.items():
        open(f"{OUT}/{name}.out", "w").write(text)
        print(f"{name:12s} {len(text):8d} bytes")
    json.dump({"sketches": len(names), "names": names, "ns": list(NS), "input_dir": "topk", "inputs": INPUTS,
               "cases": [{"name": n, "cmd": ["triangle", *SKETCH, *o]} for n, o in COMMANDS.items()]}, open(f"{OUT}/cases.json", "w"), indent=1)


if __name__ == "__main__":
    main()
