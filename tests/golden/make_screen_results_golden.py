#!/usr/bin/env python3
"""Golden outputs of the REFERENCE CLI for `mash screen` with every option of its tail
(tests/test_screen_results_model.py on the CPU, tests/test_screen_results_gpu.py on the GPU).

    make -C oracle refcli                               # oracle/_ref/mash-ref, the reference's own sources
    python tests/golden/make_screen_results_golden.py   # writes tests/golden/screen_results/{in/*, cases.json, *.out}

Every case records the set-up commands (sketches written by the same binary), the screen command and its stdout.  A
case is a PARITY case when the reference's stdout is the same on two runs and with -p 1 and -p 4, and equals the lines
of tests/screen_results_model.py; that is checked here.  One case (`full_tie`: one genome sketched under two names,
-w) may fail it: the reference gives each hash to whichever of the two its unordered_set lists first."""
import gzip, json, os, shutil, subprocess, sys, tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
from make_taxscreen_golden import ACGT, AA, CODON, fasta, mutate, reads_from

OUT = os.path.join(HERE, "screen_results")
REFCLI = os.path.join(ROOT, "oracle", "_ref", "mash-ref")


def fastq(records):
    return b"".join(b"@" + h + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for h, s in records)


def put(path, data):
    """every input is gzipped (the commands and the model read it as it is): fixtures stay small in the repository"""
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(data)


def make_inputs(d):
    rng = np.random.default_rng(20261017)
    cases = []
    rand = lambda n: ACGT[rng.integers(0, 4, n)].tobytes()
    # ---- six unrelated genomes and two relatives of the first; pools with uneven depth
    g = [rand(4000) for _ in range(6)]
    g += [mutate(rng, g[0], 0.01, ACGT), mutate(rng, g[0], 0.04, ACGT), mutate(rng, g[0], 0.16, ACGT)]    # (the last: identity below 0.9)
    put(f"{d}/plain.fa.gz", fasta([(b"gen%d genome number %d" % (i, i), s) for i, s in enumerate(g)]))
    put(f"{d}/pool_a.fa.gz", fasta(reads_from(rng, [g[0], g[0], g[0], g[2], g[6]], 300)))
    put(f"{d}/pool_b.fq.gz", fastq(reads_from(rng, [g[3], g[3], g[7]], 120)))
    sk = lambda db, out, s=200: ["sketch", "-i", "-k", "21", "-s", str(s), "-o", out, db]
    base = dict(k=21, s=200, db=["plain.fa.gz"], setup=[sk("plain.fa.gz", "plain")])
    for name, opts in [("plain", []), ("winner", ["-w"]), ("identity", ["-i", "0.9"]), ("all_rows", ["-i", "-1"]),
                       ("winner_filters", ["-w", "-i", "0.5", "-v", "0.01"])]:
        cases.append(dict(name=name, pools=["pool_a.fa.gz"], cmd=["screen", *opts, "plain.msh", "pool_a.fa.gz"], **base))
    # (k = 11: 32-bit hashes and a k-mer space small enough that unrelated rows get chance hits, with p-values above 1e-5)
    for name, opts in [("k11_plain", []), ("pvalue", ["-v", "1e-5"])]:
        cases.append(dict(name=name, k=11, s=200, db=["plain.fa.gz"], pools=["pool_a.fa.gz", "pool_b.fq.gz"], setup=[["sketch", "-i", "-k", "11", "-s", "200", "-o", "plain11", "plain.fa.gz"]],
                          cmd=["screen", *opts, "plain11.msh", "pool_a.fa.gz", "pool_b.fq.gz"]))
    cases.append(dict(name="two_files", pools=["pool_a.fa.gz", "pool_b.fq.gz"], cmd=["screen", "-w", "plain.msh", "pool_a.fa.gz", "pool_b.fq.gz"], **base))
    cases.append(dict(name="stdin", pools=["pool_b.fq.gz"], stdin="pool_b.fq.gz", cmd=["screen", "plain.msh", "-"], **base))
    # ---- a clade: 12 genomes mutated from one ancestor at 1-10 %, reads from three of them
    anc = rand(5000)
    clade = [mutate(rng, anc, r, ACGT) for r in np.linspace(0.01, 0.10, 12)]
    put(f"{d}/clade.fa.gz", fasta([(b"clade%d descendant at %d permille" % (i, 10 + 8 * i), s) for i, s in enumerate(clade)]))
    put(f"{d}/pool_clade.fa.gz", fasta(reads_from(rng, [clade[0], clade[0], clade[1], clade[2]], 400)))
    cases.append(dict(name="clade_winner", k=21, s=200, db=["clade.fa.gz"], pools=["pool_clade.fa.gz"], setup=[sk("clade.fa.gz", "clade")],
                      cmd=["screen", "-w", "clade.msh", "pool_clade.fa.gz"]))
    # ---- equal score, different length: a genome and the same genome with a run of N appended
    same = rand(3500)
    put(f"{d}/lengths.fa.gz", fasta([(b"short the genome", same), (b"other an unrelated one", rand(3500)), (b"long the genome and a run of N", same + b"N" * 500)]))
    put(f"{d}/pool_len.fa.gz", fasta(reads_from(rng, [same], 150)))
    cases.append(dict(name="length_rule", k=21, s=200, db=["lengths.fa.gz"], pools=["pool_len.fa.gz"], setup=[sk("lengths.fa.gz", "lengths")],
                      cmd=["screen", "-w", "-i", "-1", "lengths.msh", "pool_len.fa.gz"]))
    # ---- a sketch with fewer than s hashes
    put(f"{d}/small.fa.gz", fasta([(b"big four thousand bases", g[1]), (b"tiny three hundred bases", g[2][:300]), (b"mid another genome", g[4])]))
    put(f"{d}/pool_small.fa.gz", fasta(reads_from(rng, [g[2][:300], g[1]], 200)))
    cases.append(dict(name="short_sketch", k=21, s=1000, db=["small.fa.gz"], pools=["pool_small.fa.gz"], setup=[sk("small.fa.gz", "small", 1000)],
                      cmd=["screen", "-w", "small.msh", "pool_small.fa.gz"]))
    # ---- protein queries, nucleotide pool
    prot = [AA[rng.integers(0, 20, 900)].tobytes() for _ in range(3)]
    prot.append(mutate(rng, prot[0], 0.03, AA))
    put(f"{d}/prot.fa.gz", fasta([(b"prot%d protein number %d" % (i, i), s) for i, s in enumerate(prot)]))
    dna = [b"".join(CODON[a] for a in p) for p in (prot[0], prot[2])]
    put(f"{d}/pool_aa.fa.gz", fasta(reads_from(rng, dna, 160)))
    cases.append(dict(name="protein", k=9, s=200, protein=True, db=["prot.fa.gz"], pools=["pool_aa.fa.gz"],
                      setup=[["sketch", "-i", "-a", "-k", "9", "-s", "200", "-o", "prot", "prot.fa.gz"]], cmd=["screen", "-w", "prot.msh", "pool_aa.fa.gz"]))
    # ---- full tie: one genome under two names
    put(f"{d}/tie.fa.gz", fasta([(b"first one genome", same), (b"second the same genome", same), (b"third something else", rand(3500))]))
    cases.append(dict(name="full_tie", k=21, s=200, db=["tie.fa.gz"], pools=["pool_len.fa.gz"], setup=[sk("tie.fa.gz", "tie")], parity=False,
                      cmd=["screen", "-w", "-i", "-1", "tie.msh", "pool_len.fa.gz"]))
    return cases


def run_ref(case, d, threads=None):
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copytree(d, tmp, dirs_exist_ok=True)
        for s in case["setup"]:
            subprocess.run([REFCLI, *s], cwd=tmp, check=True, capture_output=True)
        cmd = list(case["cmd"])
        if threads:
            cmd[1:1] = ["-p", str(threads)]
        stdin = gzip.decompress(open(os.path.join(tmp, case["stdin"]), "rb").read()) if case.get("stdin") else None
        r = subprocess.run([REFCLI, *cmd], cwd=tmp, capture_output=True, input=stdin)
        assert r.returncode == 0, (case["name"], r.stderr[-400:])
        return r.stdout


def main():
    from oracle import pyoracle
    import screen_results_model as model
    if not os.path.exists(REFCLI):
        sys.exit("build the reference CLI first: make -C oracle refcli")
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(os.path.join(OUT, "in"))
    d = os.path.join(OUT, "in")
    cases = make_inputs(d)
    orc = pyoracle.Oracle()
    for c in cases:
        c.setdefault("parity", True)
        outs = [run_ref(c, d), run_ref(c, d), run_ref(c, d, 1), run_ref(c, d, 4)]
        stable = all(o == outs[0] for o in outs)
        open(os.path.join(OUT, c["name"] + ".out"), "wb").write(outs[0])
        same = model.case_lines(orc, c, d) == outs[0]
        print(f"{c['name']:16s} {len(outs[0].splitlines()):3d} lines  stable {stable}  reference {'==' if same else '!='} model")
        if c["parity"]:
            assert stable and same, f"{c['name']}: a parity fixture must be stable and equal to the model; reshape it"
    assert [c["name"] for c in cases if not c["parity"]] == ["full_tie"]
    with open(os.path.join(OUT, "cases.json"), "w") as f:                  # one case per line
        f.write('{"screen": [\n' + ",\n".join(json.dumps(c) for c in cases) + "\n]}\n")
    print("wrote", len(cases), "cases to", OUT)


if __name__ == "__main__":
    main()
