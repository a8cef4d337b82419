"""Pure-Python model of `mash taxscreen`: the specification the GPU tests are judged by.

Two levels.
  * Node level (what libmashgpu computes): a forest over dense node indices, the LCA node of every distinct
    database hash, the per-node histograms and the clade sums.  `hash_nodes`, `taxon_counts`.
  * Report level (what the command prints): NCBI dump parsing, taxID assignment, the reference's
    getLowestCommonAncestor over taxIDs with its special answers (taxID 1 for anything that meets at a root or
    involves a taxID the taxonomy does not hold), and the Kraken-style report.  `report`.

The clade sums are the INTENDED ones: every taxon's own counts are added exactly once to itself and to each of its
ancestors.  The reference inserts into the unordered_map it iterates in that loop and, when the map rehashes, visits
entries twice or not at all; tests/test_taxscreen_model.py keeps one recorded fixture that shows it."""
import gzip

NONE = 0xFFFFFFFF          # MG_TAX_NONE
DISJOINT = 0xFFFFFFFE      # MG_TAX_DISJOINT


# ------------------------------------------------------------------------------------------------ node level
def depths(parent):
    depth = [None] * len(parent)
    for i in range(len(parent)):
        path, v = [], i
        while depth[v] is None and parent[v] != v:
            path.append(v)
            v = parent[v]
            assert len(path) <= len(parent), "cycle"
        if depth[v] is None:
            depth[v] = 0
        d = depth[v]
        for u in reversed(path):
            d += 1
            depth[u] = d
    return depth


def lca(parent, depth, a, b):
    if a == NONE or a == b:
        return b
    if b == NONE:
        return a
    if DISJOINT in (a, b):
        return DISJOINT
    while depth[a] > depth[b]:
        a = parent[a]
    while depth[b] > depth[a]:
        b = parent[b]
    while a != b:
        if parent[a] == a:
            return DISJOINT
        a, b = parent[a], parent[b]
    return a


def hash_nodes(parent, rows, row_node):
    """rows: per database row its hashes; -> {hash: node}"""
    depth = depths(parent)
    out = {}
    for hashes, node in zip(rows, row_node):
        for h in hashes:
            h = int(h)
            out[h] = lca(parent, depth, out.get(h, NONE), int(node))
    return out


def taxon_counts(parent, hash_node, observed):
    """-> ([(node, tax_count, tax_hash_count, clade_count, clade_hash_count)] ordered by node, nodes with
    clade_hash_count > 0 only, DISJOINT and NONE last and each its own clade; total_count; total_hash_count)"""
    own = {}
    for h, node in hash_node.items():
        c = own.setdefault(node, [0, 0])
        c[1] += 1
        if h in observed:
            c[0] += 1
    clade = {}
    for node, (tc, thc) in own.items():
        v = node
        while True:
            c = clade.setdefault(v, [0, 0])
            c[0] += tc
            c[1] += thc
            if v >= DISJOINT or parent[v] == v:
                break
            v = parent[v]
    rows = [(v, own.get(v, [0, 0])[0], own.get(v, [0, 0])[1], c[0], c[1]) for v, c in sorted(clade.items()) if c[1] > 0]
    return rows, sum(c[0] for c in own.values()), sum(c[1] for c in own.values())


# ---------------------------------------------------------------------------------------------- report level
def parse_taxonomy(nodes_path, names_path):
    """-> {taxid: [parent taxid or None, rank, scientific name]}; a node whose parent is itself (or is missing from the
    file) is a root"""
    tax = {}
    for line in open(nodes_path, encoding="utf-8"):
        f = line.rstrip("\n").split("\t|")
        if len(f) < 3:
            continue
        t = int(f[0])
        if t not in tax:
            tax[t] = [int(f[1]), f[2].lstrip("\t"), ""]
    for t, e in tax.items():
        if e[0] == t or e[0] not in tax:
            e[0] = None
    for line in open(names_path, encoding="utf-8"):
        f = line.rstrip("\n").split("\t|")
        if len(f) >= 4 and f[3].lstrip("\t") == "scientific name" and int(f[0]) in tax:
            tax[int(f[0])][2] = f[1].lstrip("\t")
    return tax


def reference_taxids(names, comments, mapping_path=None):
    """mapping file first (<taxid><one separator char><name to end of line>; the first line of a name wins), else the
    last `taxid <n>` word pair of the comment, else 0"""
    by_name = {}
    if mapping_path:
        for line in open(mapping_path, encoding="utf-8"):
            line = line.rstrip("\n").lstrip()
            digits = 0
            while digits < len(line) and line[digits].isdigit():
                digits += 1
            if digits == 0:
                break
            by_name.setdefault(line[digits + 1:], int(line[:digits]))
    out = []
    for name, comment in zip(names, comments):
        t = by_name.get(name, 0)
        if t == 0:
            words = comment.split()
            i = 0
            while i < len(words):
                if words[i] == "taxid":
                    i += 1
                    if i < len(words) and words[i].isdigit():
                        t = int(words[i])
                    else:
                        t = 0
                        break
                i += 1
        out.append(t)
    return out


def ref_lca(tax, a, b):
    """TaxDB::getLowestCommonAncestor as the reference behaves, taxIDs in and out"""
    if b == 0:
        return a
    if a == 0:
        return b
    if a not in tax or b not in tax:
        return 1
    path, x = set(), a
    while x is not None and x > 1 and tax[x][0] is not None:
        if x == b:
            return b
        path.add(x)
        x = tax[x][0]
    y = b
    while y > 0 and tax[y][0] is not None:
        if y in path:
            return y
        y = tax[y][0]
    return 1


def report_counts(tax, row_taxids, rows, observed):
    """-> ({taxid: [clade_count, tax_count, tax_hash_count, clade_hash_count, children]}, total_count, total_hash_count)"""
    hash_tax = {}
    for hashes, t in zip(rows, row_taxids):
        for h in hashes:
            h = int(h)
            hash_tax[h] = ref_lca(tax, t, hash_tax.get(h, 0))
    counts = {}
    for h, t in hash_tax.items():
        c = counts.setdefault(t, [0, 0, 0, 0, set()])
        c[2] += 1
        if h in observed:
            c[1] += 1
    total = sum(c[1] for c in counts.values())
    total_hash = sum(c[2] for c in counts.values())
    for t, (_, tc, thc, _, _) in list(counts.items()):
        v = t if t in tax else None
        while v is not None:
            c = counts.setdefault(v, [0, 0, 0, 0, set()])
            c[0] += tc
            c[3] += thc
            p = tax[v][0]
            if p is not None:
                counts.setdefault(p, [0, 0, 0, 0, set()])[4].add(v)
            v = p
    return counts, total, total_hash


def report(tax, row_taxids, rows, observed):
    """the bytes `mash taxscreen` prints"""
    counts, total, _ = report_counts(tax, row_taxids, rows, observed)
    out = ["%\thashes\ttaxHashes\thashesDB\ttaxHashesDB\ttaxID\trank\tname\n"]

    def walk(t, depth):
        c = counts.get(t)
        if c is None or c[0] == 0:
            return
        out.append("%.4f\t%d\t%d\t%d\t%d\t%s\t%d\t%s%s\n" % (100 * c[0] / total, c[0], c[1], c[3], c[2], tax[t][1], t, "  " * depth, tax[t][2]))
        for ch in sorted(c[4], key=lambda x: (-counts[x][0], x)):
            walk(ch, depth + 1)

    walk(1, 0)
    return "".join(out).encode()


# -------------------------------------------------------------------------------------------------- file helpers
def read_fastx(path):
    """[(name, comment, sequence bytes)] of a FASTA / FASTQ file, gzipped or not"""
    raw = open(path, "rb").read()
    if raw[:2] == b"\x1f\x8b":
        raw = gzip.decompress(raw)
    recs, lines, i = [], raw.split(b"\n"), 0
    while i < len(lines):
        ln = lines[i]
        if ln[:1] == b">":
            head, seq = ln[1:], []
            i += 1
            while i < len(lines) and lines[i][:1] != b">":
                seq.append(lines[i].strip())
                i += 1
            name, _, comment = head.decode().partition(" ")
            recs.append((name, comment, b"".join(seq)))
        elif ln[:1] == b"@":
            name, _, comment = ln[1:].decode().partition(" ")
            recs.append((name, comment, lines[i + 1].strip()))
            i += 4
        else:
            i += 1
    return recs


PROTEIN = "ACDEFGHIKLMNPQRSTVWY"


def fixture_sets(orc, case, indir):
    """For a case of tests/golden/taxscreen/cases.json: (names, comments, rows, observed) -- the database records with
    their bottom-s hashes and the set of k-mer hashes of the pool, both from the CPU oracle"""
    import os
    import numpy as np
    aa = bool(case.get("protein"))
    k, s = case["k"], case["s"]
    p = orc.params(k=k, s=s, alphabet=PROTEIN if aa else "ACGT", noncanonical=aa)
    recs = read_fastx(os.path.join(indir, case["db"]))
    rows = [orc.sketch_records([seq], p)[0] for _, _, seq in recs]
    observed = set()
    for pool in case["pools"]:
        for _, _, seq in read_fastx(os.path.join(indir, pool)):
            if len(seq) < k:
                continue
            parts = orc.six_frames(seq) if aa else [seq]
            for part in parts:
                if len(part) < k:
                    continue
                b = np.frombuffer(bytes(part), dtype=np.uint8).copy()
                observed.update(int(x) for x in orc.kmer_hashes(b, np.array([0, len(b)], dtype=np.uint64), p))
    return [r[0] for r in recs], [r[1] for r in recs], rows, observed
