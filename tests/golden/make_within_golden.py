#!/usr/bin/env python3
"""Recorded stdout and exit status of the REFERENCE CLI for `mash within` (tests/test_within_model.py, tests/test_within_gpu.py).

    make -C oracle refcli                        # oracle/_ref/mash-ref and its objects, from the reference's unmodified sources
    python tests/golden/make_within_golden.py    # writes tests/golden/within/{*.fa.gz, *.msh, *.txt, *.out, cases.json}

The reference compiles CommandContain.cpp always but registers the command only under COMMAND_WITHIN, so this script compiles
the reference's mash.cpp once more with that macro and links it against the objects `refcli` left: oracle/_ref/mash-ref-within
(git-ignored like everything under oracle/_ref).  No test needs that binary; tests read the recordings.

The inputs (k = 16, so hashes are 32-bit; a few kbp): references r_genome (6 kbp), r_other (unrelated, 3 kbp), r_short (a
100-base piece of the genome: fewer hashes than any sketch size used) and r_tiny (16 bases: one hash); queries: the genome
itself, clean and mutated pieces of it, an unrelated sequence, a 300-base piece (its hashes span the whole range, so a
reference sketch is exhausted long before it) and two tiny ones (20 and 16 bases).  The .msh files are the reference's own
`mash sketch` of these at other sketch sizes.

Conditions on the recording, asserted here (the seed is the first that meets them) and again by the test on the text alone:
  * the scores 0 and 1 and a score strictly between occur;
  * some pair is absent even under -e 1 (j = 0);
  * some pair passes -e 1 and not -e 0.3, some passes -e 0.3 and not -e 0.05;
and, under tests/within_model.py, the pairs of the cases end their walk in all three ways (by |Q|, by |R|, by exhaustion of R).
Never run by a test; only data is committed."""
import glob, gzip, json, os, subprocess, sys, tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import within_model as wm  # noqa: E402

OUT = os.path.join(HERE, "within")
ORACLE = os.path.join(ROOT, "oracle")
# where the reference's sources lie: $REF, else what oracle/Makefile says (its `REF ?=` line)
REF = os.environ.get("REF") or next(l.split("?=")[1].strip() for l in open(os.path.join(ORACLE, "Makefile")) if l.startswith("REF"))
REFCLI = os.path.join(ORACLE, "_ref", "mash-ref-within")
K = 16
SK = ["-i", "-k", str(K)]

# sketches the reference CLI writes before the cases run: name -> (source, sketch size)
SKETCHES = {"ref_s1000": ("ref.fa.gz", 1000), "ref_s200": ("ref.fa.gz", 200), "q_s64": ("queries.fa.gz", 64), "q_s2000": ("queries.fa.gz", 2000)}
# the cases: arguments after `within`; `sets` says what the model needs: per input its source, its sketch size and whether
# every sequence is a sketch of its own (-i)
CASES = [
    ("fa_e005", [*SK, "-s", "1000", "ref.fa.gz", "queries.fa.gz"], 1000),
    ("fa_e03", [*SK, "-s", "1000", "-e", "0.3", "ref.fa.gz", "queries.fa.gz"], 1000),
    ("fa_e1", [*SK, "-s", "1000", "-e", "1", "ref.fa.gz", "queries.fa.gz"], 1000),
    ("fa_s200_e1_p3", [*SK, "-s", "200", "-e", "1", "-p", "3", "ref.fa.gz", "queries.fa.gz"], 200),
    ("fa_whole_files_e1", ["-k", str(K), "-s", "400", "-e", "1", "ref.fa.gz", "queries.fa.gz", "ref.fa.gz"], 400),
    ("msh_ref_e03", ["-i", "-e", "0.3", "ref_s1000.msh", "queries.fa.gz"], 1000),
    ("msh_ref_s200_e1", ["-i", "-e", "1", "ref_s200.msh", "queries.fa.gz"], 200),
    ("msh_smaller_queries_e1", ["-e", "1", "ref_s1000.msh", "q_s64.msh"], 1000),
    ("msh_larger_queries_e005", ["ref_s1000.msh", "q_s2000.msh"], 1000),
    ("msh_both_e03", ["-e", "0.3", "ref_s200.msh", "q_s64.msh", "q_s2000.msh"], 200),
    ("list_e03", ["-l", "-i", "-e", "0.3", "ref_s1000.msh", "queries.txt"], 1000),
    ("quirk_a_continues", ["-a", "-i", "-e", "1", "ref_s1000.msh", "queries.fa.gz"], 1000),
    ("quirk_z_continues", ["-z", "ACGT", "-i", "-e", "1", "ref_s1000.msh", "queries.fa.gz"], 1000),
    ("refuses_k", ["-k", "16", "-i", "ref_s1000.msh", "queries.fa.gz"], 1000),
    ("refuses_n", ["-n", "-i", "ref_s1000.msh", "queries.fa.gz"], 1000),
]
LISTS = {"queries.txt": ["queries.fa.gz", "q_s64.msh"]}


def build_refcli():
    if os.path.exists(REFCLI):
        return
    cli = os.path.join(ORACLE, "_ref", "cli")
    if not os.path.exists(os.path.join(cli, "CommandContain.o")):
        sys.exit("build the reference CLI first: make -C oracle refcli")
    obj = os.path.join(cli, "mash_within.o")
    subprocess.run(["g++", "-O2", "-std=c++14", "-include", "limits", "-w", "-Ishim", "-I../mash_amd/host", f"-I{REF}/src", f"-I{REF}/src/mash",
                    "-DCOMMAND_WITHIN", "-c", f"{REF}/src/mash/mash.cpp", "-o", obj], cwd=ORACLE, check=True)
    objs = [o for o in sorted(glob.glob(os.path.join(cli, "*.o"))) if os.path.basename(o) != "mash.o"]
    subprocess.run(["g++", "-o", REFCLI, *objs, "-lz", "-lpthread", "-lm"], check=True)


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


def inputs(seed):
    rng = np.random.default_rng(seed)
    g = rand_dna(rng, 6000)
    other = rand_dna(rng, 3000)
    refs = [(b"r_genome the genome", g), (b"r_other unrelated", other), (b"r_short a piece of 100", g[2000:2100]), (b"r_tiny one k-mer", rand_dna(rng, 16))]
    qrys = [(b"q_genome the genome itself", g), (b"q_half a clean half", g[1000:4000]), (b"q_mut a mutated half", mutate(rng, g[2500:5500], 0.03)),
            (b"q_alien unrelated", rand_dna(rng, 2500)), (b"q_piece 300 clean bases", g[4000:4300]), (b"q_piece_mut 300 mutated bases", mutate(rng, g[500:800], 0.02)),
            (b"q_five five k-mers", rand_dna(rng, 20)), (b"q_one one k-mer", rand_dna(rng, 16))]
    return refs, qrys


def record(d, seed):
    refs, qrys = inputs(seed)
    for f, recs in (("ref.fa.gz", refs), ("queries.fa.gz", qrys)):
        with gzip.GzipFile(f"{d}/{f}", "wb", mtime=0) as z:
            z.write(fasta(recs))
    for f, lines in LISTS.items():
        open(f"{d}/{f}", "w").write("".join(x + "\n" for x in lines))
    for name, (src, s) in SKETCHES.items():
        subprocess.run([REFCLI, "sketch", *SK, "-s", str(s), "-o", name, src], cwd=d, capture_output=True, check=True, timeout=120)
    outs = {}
    for name, args, _ in CASES:
        r = subprocess.run([REFCLI, "within", *args], cwd=d, capture_output=True, timeout=120)
        outs[name] = (r.stdout.decode(), r.returncode, r.stderr.decode())
    return outs


def text_conditions(outs):
    """the conditions the test asserts again on the text alone: (met, why not)"""
    e005, e03, e1 = (wm.parse(outs[n][0]) for n in ("fa_e005", "fa_e03", "fa_e1"))
    scores = {float(l[0]) for l in e1}
    if 0.0 not in scores or 1.0 not in scores or not any(0 < x < 1 for x in scores):
        return False, "scores 0, 1 and one between do not all occur"
    if len(e1) >= 4 * 8:
        return False, "no pair is absent under -e 1"
    pairs = lambda ls: {(l[2], l[3]) for l in ls}
    if not pairs(e1) - pairs(e03) or not pairs(e03) - pairs(e005) or not pairs(e005):
        return False, "the thresholds do not separate the pairs"
    if outs["refuses_k"][1] != 1 or outs["refuses_n"][1] != 1 or outs["quirk_a_continues"][1] != 0 or not outs["quirk_a_continues"][0]:
        return False, "refusals"
    return True, ""


def model_conditions(d):
    """all three terminations among the pairs of the FASTA cases (sketches by the oracle)"""
    from tests.within_fixture import sketch_fasta
    seen = set()
    for s in (1000, 200):
        refs, qrys = sketch_fasta(f"{d}/ref.fa.gz", K, s, True), sketch_fasta(f"{d}/queries.fa.gz", K, s, True)
        seen |= {wm.termination(r, q) for _, r in refs for _, q in qrys}
    return {"Q", "R", "exhausted"} <= seen, f"terminations seen: {sorted(seen)}"


def main():
    build_refcli()
    os.makedirs(OUT, exist_ok=True)
    for seed in range(20261021, 20261021 + 200):
        with tempfile.TemporaryDirectory(prefix="withingold_") as d:
            outs = record(d, seed)
            ok, why = text_conditions(outs)
            if ok:
                ok, why = model_conditions(d)
            print(f"seed {seed}: {'ok' if ok else why}")
            if not ok:
                continue
            for f in ["ref.fa.gz", "queries.fa.gz", *LISTS, *(n + ".msh" for n in SKETCHES)]:
                open(f"{OUT}/{f}", "wb").write(open(f"{d}/{f}", "rb").read())
            for name, (text, _, _) in outs.items():
                open(f"{OUT}/{name}.out", "w").write(text)
                print(f"{name:28s} {len(text):6d} bytes, exit {outs[name][1]}")
            json.dump({"seed": seed, "k": K, "sketches": {n: {"source": src, "s": s} for n, (src, s) in SKETCHES.items()}, "lists": LISTS,
                       "cases": [{"name": n, "cmd": ["within", *a], "s": s, "exit": outs[n][1]} for n, a, s in CASES]},
                      open(f"{OUT}/cases.json", "w"), indent=1)
            return
    sys.exit("no seed met the conditions")


if __name__ == "__main__":
    main()
