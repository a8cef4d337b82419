#!/usr/bin/env python3
"""Golden outputs of the REFERENCE CLI for `mash taxscreen` and `mash bounds`
(tests/test_taxscreen_model.py on the CPU, tests/test_taxscreen_gpu.py on the GPU).

    make -C oracle refcli                          # oracle/_ref/mash-ref, the reference's own sources
    python tests/golden/make_taxscreen_golden.py   # writes tests/golden/taxscreen/{in/*, cases.json, *.out}

Synthetic genomes descend from each other along a synthetic taxonomy (a child's genome is its parent's with
substitutions), so hashes are shared at every level and LCAs land on inner nodes.  Every case records the set-up
commands (sketches written by the same binary), the taxscreen command and its stdout.  A case is a PARITY case when
the reference's stdout equals the report of tests/taxscreen_model.py; that is checked here, and at most one case
(`defect`: the reference's clade loop counting twice, see the model's docstring) may fail it."""
import gzip, json, os, shutil, subprocess, sys, tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(HERE, "taxscreen")
REFCLI = os.path.join(ROOT, "oracle", "_ref", "mash-ref")
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
CODON = {a: c for a, c in zip(b"ACDEFGHIKLMNPQRSTVWY", [b"GCT", b"TGC", b"GAC", b"GAA", b"TTC", b"GGA", b"CAC", b"ATC", b"AAG", b"CTG", b"ATG",
                                                        b"AAC", b"CCA", b"CAG", b"CGT", b"TCA", b"ACC", b"GTG", b"TGG", b"TAC"])}


def mutate(rng, seq, rate, letters):
    a = np.frombuffer(seq, dtype=np.uint8).copy()
    idx = np.nonzero(rng.random(len(a)) < rate)[0]
    a[idx] = letters[rng.integers(0, len(letters), len(idx))]
    return a.tobytes()


def fasta(records, width=70):
    out = []
    for head, seq in records:
        out.append(b">" + head + b"\n")
        out += [seq[i:i + width] + b"\n" for i in range(0, len(seq), width)]
    return b"".join(out)


def taxonomy(shape):
    """{taxid: parent taxid}, leaves; taxID 1 is the root"""
    parent, level, nxt = {1: 1}, [1], 2
    for step in shape:                       # step = children per node at this level (1: a single-child chain link)
        new = []
        for v in level:
            for _ in range(step):
                parent[nxt] = v
                new.append(nxt)
                nxt += 1
        level = new
    return parent, level


def write_taxonomy(d, parent, skip=()):
    os.makedirs(d, exist_ok=True)
    ranks = ["no rank", "superkingdom", "phylum", "class", "order", "family", "genus", "species", "strain"]
    depth = {1: 0}
    for t in sorted(parent):
        if t != 1:
            depth[t] = depth[parent[t]] + 1
    with open(os.path.join(d, "nodes.dmp"), "w") as f:
        for t in sorted(parent):
            if t not in skip:
                f.write(f"{t}\t|\t{parent[t]}\t|\t{ranks[min(depth[t], len(ranks) - 1)]}\t|\tXX\t|\t0\t|\n")
    with open(os.path.join(d, "names.dmp"), "w") as f:
        for t in sorted(parent):
            if t in skip:
                continue
            if t % 3 == 0:
                f.write(f"{t}\t|\told name of {t}\t|\t\t|\tsynonym\t|\n")
            f.write(f"{t}\t|\t{'root' if t == 1 else 'Taxon number %d' % t}\t|\t\t|\tscientific name\t|\n")


def genomes_along(rng, parent, length, rate, letters):
    g = {1: letters[rng.integers(0, len(letters), length)].tobytes()}
    for t in sorted(parent):
        if t != 1:
            g[t] = mutate(rng, g[parent[t]], rate, letters)
    return g


def reads_from(rng, seqs, n, length=150):
    out = []
    for i in range(n):
        src = seqs[i % len(seqs)]
        o = int(rng.integers(0, len(src) - length))
        out.append((b"read%d" % i, src[o:o + length]))
    return out


def make_inputs(d):
    rng = np.random.default_rng(20261016)
    cases = []
    # ---- balanced binary taxonomy, 8 leaves; references on the leaves and on two inner nodes
    par, leaves = taxonomy([2, 2, 2])
    write_taxonomy(f"{d}/tax_bal", par)
    write_taxonomy(f"{d}/tax_bal_gap", par, skip=(leaves[5],))          # one leaf's taxID is not in nodes.dmp
    g = genomes_along(rng, par, 3000, 0.02, ACGT)
    refs = leaves + [4, 7]
    recs = [(b"ref%d genome of taxon %d taxid %d" % (i, t, t), g[t]) for i, t in enumerate(refs)]
    with gzip.GzipFile(f"{d}/bal.fa.gz", "wb", mtime=0) as f:
        f.write(fasta(recs))
    open(f"{d}/bal.map", "w").write("".join(f"{t}\tref{i}\n" for i, t in enumerate(refs)))
    open(f"{d}/bal_some.map", "w").write("".join(f"{t} ref{i}\n" for i, t in enumerate(refs) if i % 3))   # every third reference unmapped
    # (comments without the taxid words for the database that has to rely on the mapping file)
    with gzip.GzipFile(f"{d}/bal_plain.fa.gz", "wb", mtime=0) as f:
        f.write(fasta([(b"ref%d plain" % i, g[t]) for i, t in enumerate(refs)]))
    # comment-carried taxIDs for the even references only, a decoy pair first ("taxid 2 ... taxid <t>": the last one wins)
    with gzip.GzipFile(f"{d}/bal_mixed.fa.gz", "wb", mtime=0) as f:
        f.write(fasta([(b"ref%d%s" % (i, b" from taxid 2 really taxid %d" % t if i % 2 == 0 else b" nothing here"), g[t]) for i, t in enumerate(refs)]))
    open(f"{d}/bal_odd.map", "w").write("".join(f"{t}\tref{i}\n" for i, t in enumerate(refs) if i % 2 == 1 and i != 5))   # ref5: neither
    src = [g[t] for t in leaves[::3]]
    open(f"{d}/pool_a.fa", "wb").write(fasta(reads_from(rng, src, 240)))
    open(f"{d}/pool_b.fa", "wb").write(fasta(reads_from(rng, [g[leaves[1]]], 80)))
    with gzip.GzipFile(f"{d}/pool_c.fa.gz", "wb", mtime=0) as f:
        f.write(fasta(reads_from(rng, [g[leaves[6]], g[7]], 80)))
    open(f"{d}/pool_none.fa", "wb").write(fasta(reads_from(rng, [ACGT[rng.integers(0, 4, 4000)].tobytes()], 60)))
    sk = lambda db, out: ["sketch", "-i", "-k", "21", "-s", "200", "-o", out, db]
    base = dict(k=21, s=200)
    cases.append(dict(name="balanced", db="bal_plain.fa.gz", pools=["pool_a.fa"], taxdir="tax_bal", mapping="bal.map", **base,
                      setup=[sk("bal_plain.fa.gz", "bal_plain")], cmd=["taxscreen", "-m", "bal.map", "-t", "tax_bal", "bal_plain.msh", "pool_a.fa"]))
    cases.append(dict(name="comment_taxids", db="bal.fa.gz", pools=["pool_a.fa"], taxdir="tax_bal", mapping=None, **base,
                      setup=[sk("bal.fa.gz", "bal")], cmd=["taxscreen", "-t", "tax_bal", "-p", "4", "-i", "0.9", "-v", "0.01", "bal.msh", "pool_a.fa"]))
    cases.append(dict(name="no_taxid", db="bal_plain.fa.gz", pools=["pool_a.fa"], taxdir="tax_bal", mapping="bal_some.map", **base,
                      setup=[sk("bal_plain.fa.gz", "bal_plain")], cmd=["taxscreen", "-m", "bal_some.map", "-t", "tax_bal", "bal_plain.msh", "pool_a.fa"]))
    cases.append(dict(name="unknown_taxid", db="bal.fa.gz", pools=["pool_a.fa", "pool_b.fa"], taxdir="tax_bal_gap", mapping=None, **base,
                      setup=[sk("bal.fa.gz", "bal")], cmd=["taxscreen", "-t", "tax_bal_gap", "bal.msh", "pool_a.fa", "pool_b.fa"]))
    cases.append(dict(name="three_pools", db="bal.fa.gz", pools=["pool_a.fa", "pool_b.fa", "pool_c.fa.gz"], taxdir="tax_bal", mapping=None, **base,
                      setup=[sk("bal.fa.gz", "bal")], cmd=["taxscreen", "-t", "tax_bal", "bal.msh", "pool_a.fa", "pool_b.fa", "pool_c.fa.gz"]))
    cases.append(dict(name="no_hits", db="bal.fa.gz", pools=["pool_none.fa"], taxdir="tax_bal", mapping=None, **base,
                      setup=[sk("bal.fa.gz", "bal")], cmd=["taxscreen", "-t", "tax_bal", "bal.msh", "pool_none.fa"]))
    cases.append(dict(name="mapping_and_comments", db="bal_mixed.fa.gz", pools=["pool_a.fa", "pool_c.fa.gz"], taxdir="tax_bal", mapping="bal_odd.map", **base,
                      setup=[sk("bal_mixed.fa.gz", "bal_mixed")],
                      cmd=["taxscreen", "-m", "bal_odd.map", "-t", "tax_bal", "bal_mixed.msh", "pool_a.fa", "pool_c.fa.gz"]))
    # ---- amino-acid database, nucleotide pool translated in six frames
    par, leaves = taxonomy([2, 3])
    write_taxonomy(f"{d}/tax_aa", par)
    g = genomes_along(rng, par, 900, 0.03, AA)
    with gzip.GzipFile(f"{d}/prot.fa.gz", "wb", mtime=0) as f:
        f.write(fasta([(b"prot%d taxid %d" % (i, t), g[t]) for i, t in enumerate(leaves + [2])]))
    dna = [b"".join(CODON[a] for a in g[t]) for t in leaves[::2]]
    open(f"{d}/pool_aa.fa", "wb").write(fasta(reads_from(rng, dna, 150)))
    cases.append(dict(name="protein_six_frames", db="prot.fa.gz", pools=["pool_aa.fa"], taxdir="tax_aa", mapping=None, k=9, s=200, protein=True,
                      setup=[["sketch", "-i", "-a", "-k", "9", "-s", "200", "-o", "prot", "prot.fa.gz"]],
                      cmd=["taxscreen", "-t", "tax_aa", "prot.msh", "pool_aa.fa"]))
    # ---- the defect: binary for 4 levels, then 5-level single-child chains -- ancestors that are no hash's LCA enter the
    #      reference's map while it is being iterated
    par, leaves = taxonomy([2, 2, 2, 2, 1, 1, 1, 1, 1])
    write_taxonomy(f"{d}/tax_chain", par)
    g = genomes_along(rng, par, 2500, 0.012, ACGT)
    with gzip.GzipFile(f"{d}/chain.fa.gz", "wb", mtime=0) as f:
        f.write(fasta([(b"leaf%d taxid %d" % (i, t), g[t]) for i, t in enumerate(leaves)]))
    open(f"{d}/pool_chain.fa", "wb").write(fasta(reads_from(rng, [g[t] for t in leaves[::3]], 200)))
    cases.append(dict(name="defect", db="chain.fa.gz", pools=["pool_chain.fa"], taxdir="tax_chain", mapping=None, k=21, s=200, parity=False,
                      setup=[["sketch", "-i", "-k", "21", "-s", "200", "-o", "chain", "chain.fa.gz"]],
                      cmd=["taxscreen", "-t", "tax_chain", "chain.msh", "pool_chain.fa"]))
    return cases


def main():
    from oracle import pyoracle
    import taxscreen_model as model
    if not os.path.exists(REFCLI):
        sys.exit("build the reference CLI first: make -C oracle refcli")
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(os.path.join(OUT, "in"))
    d = os.path.join(OUT, "in")
    cases = make_inputs(d)
    orc = pyoracle.Oracle()
    excluded = []
    for c in cases:
        c.setdefault("parity", True)
        with tempfile.TemporaryDirectory() as tmp:
            shutil.copytree(d, tmp, dirs_exist_ok=True)
            for s in c["setup"]:
                subprocess.run([REFCLI, *s], cwd=tmp, check=True, capture_output=True)
            r = subprocess.run([REFCLI, *c["cmd"]], cwd=tmp, capture_output=True)
            assert r.returncode == 0, (c["name"], r.stderr[-400:])
        open(os.path.join(OUT, c["name"] + ".out"), "wb").write(r.stdout)
        names, comments, rows, observed = model.fixture_sets(orc, c, d)
        tax = model.parse_taxonomy(os.path.join(d, c["taxdir"], "nodes.dmp"), os.path.join(d, c["taxdir"], "names.dmp"))
        ids = model.reference_taxids(names, comments, os.path.join(d, c["mapping"]) if c["mapping"] else None)
        same = model.report(tax, ids, rows, observed) == r.stdout
        print(f"{c['name']:24s} {len(r.stdout.splitlines()):4d} lines  reference {'==' if same else '!='} model")
        if c["parity"]:
            assert same, f"{c['name']}: a parity fixture must be one where reference and model agree; reshape it"
        else:
            assert not same, f"{c['name']}: meant to show the reference's defect, but the reference agrees with the model"
            excluded.append(c["name"])
    assert len(excluded) <= 1
    # ---- mash bounds: no inputs
    bounds = [dict(name="bounds_default", cmd=["bounds"]), dict(name="bounds_k16_p95", cmd=["bounds", "-k", "16", "-p", "0.95"])]
    for b in bounds:
        r = subprocess.run([REFCLI, *b["cmd"]], capture_output=True, check=True)
        open(os.path.join(OUT, b["name"] + ".out"), "wb").write(r.stdout)
    json.dump(dict(taxscreen=cases, bounds=bounds), open(os.path.join(OUT, "cases.json"), "w"), indent=1)
    print("wrote", len(cases), "taxscreen cases and", len(bounds), "bounds cases to", OUT)


if __name__ == "__main__":
    main()
