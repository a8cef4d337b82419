"""Shared test helpers (pure Python, CPU)."""
import gzip
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def read_fastx(path):
    """Minimal FASTA/FASTQ reader with kseq.h semantics (kseq.h:171-208): header
    char > or @, name up to first whitespace, comment = rest of line, sequence =
    all isgraph bytes up to the next >, @ or + line start.  Returns
    [(name, comment, seq bytes)]."""
    op = gzip.open if path.endswith(".gz") else open
    with op(path, "rb") as f:
        data = f.read()
    recs = []
    lines = data.split(b"\n")
    i = 0
    n = len(lines)
    while i < n:
        ln = lines[i]
        if not ln or ln[:1] not in (b">", b"@"):
            i += 1
            continue
        hdr = ln[1:]
        parts = hdr.split(None, 1)
        name = parts[0] if parts else b""
        comment = parts[1] if len(parts) > 1 else b""
        i += 1
        seq = bytearray()
        while i < n and lines[i][:1] not in (b">", b"@", b"+"):
            seq += bytes(c for c in lines[i] if 33 <= c <= 126)
            i += 1
        if i < n and lines[i][:1] == b"+":
            i += 1
            q = 0
            while i < n and q < len(seq):
                q += len(lines[i])
                i += 1
        recs.append((name, comment, bytes(seq)))
    return recs


def round_robin(lists):
    """Interleave records of several files the way sketchFile does (Sketch.cpp:1200-1270)."""
    out = []
    iters = [iter(l) for l in lists]
    while iters:
        nxt = []
        for it in iters:
            try:
                out.append(next(it))
                nxt.append(it)
            except StopIteration:
                pass
        iters = nxt
    return out


def fmt_g(x):
    """ostream << double with default precision (6 significant digits, %g style)."""
    return "%g" % x


def load_golden_genomes():
    z = np.load(os.path.join(GOLDEN, "genomes_sketches.npz"))
    return z["hashes"], z["lengths"], [str(s) for s in z["names"]]


def load_golden_reads():
    z = np.load(os.path.join(GOLDEN, "reads_sketch.npz"))
    return z["hashes"], int(z["length"]), str(z["comment"])


def load_ref_sketch_vectors(name="ref_sketch_vectors.npz"):
    z = np.load(os.path.join(GOLDEN, name))
    cfgs = json.loads(str(z["cfgs"]))
    out = []
    for c in cfgs:
        i = c["idx"]
        bases = z[f"bases_{i}"].tobytes()
        lens = z[f"reclen_{i}"]
        recs, o = [], 0
        for l in lens:
            recs.append(bases[o:o + int(l)])
            o += int(l)
        out.append((c, recs, z[f"hashes_{i}"], z[f"counts_{i}"]))
    return out


# ---------------------------------------------------------------------------------------------- rect jobs against the oracle

COUNTS = np.dtype([("numer", "<u4"), ("denom", "<u4")])          # mg_counts
PAD = np.uint64(0xFFFFFFFFFFFFFFFF)


def rect_oracle(oracle, rt, rn, rl, qt, qn, ql, k, kspace):
    """`mash dist` of the query table against the reference table by the oracle: (numer, denom, distance, p_value) as
    [nq, nref] arrays.  Both tables are cut to s = min(s_ref, s_qry) columns (CommandDistance.cpp:313-315) with nhash
    clamped to s, the queries are stacked under the references, and rows [nref, nref + nq) of that table's triangle
    are computed: the first nref columns of such a row are the query against every reference."""
    nref, nq = len(rn), len(qn)
    s = min(rt.shape[1], qt.shape[1])
    table = np.ascontiguousarray(np.concatenate([rt[:, :s], qt[:, :s]]), dtype=np.uint64)
    nhash = np.minimum(np.concatenate([rn, qn]), s).astype(np.uint32)
    lengths = np.concatenate([rl, ql]).astype(np.uint64)
    flat = oracle.triangle(table, nhash, lengths, nref, nref + nq, k, kspace, stats=True)
    i = np.arange(nq, dtype=np.int64)
    idx = (nref * i + i * (i - 1) // 2)[:, None] + np.arange(nref, dtype=np.int64)[None, :]     # row nref + i holds nref + i pairs
    return tuple(np.ascontiguousarray(a[idx]) for a in flat)


def expand_rect(edges, rn, qn, s, q_begin, q_end, nref):
    """The dense counts of queries [q_begin, q_end) out of mg_compare_rect_sparse_host's exceptions (include/mashgpu.h):
    every pair is {0, min(s, |A| + |B|)} with |X| = min(nhash, s), except the pairs listed in `edges`
    ({row = query index in the query table, col = reference index, numer, denom})."""
    q_end = min(q_end, len(qn))
    nrows = max(q_end - q_begin, 0)
    out = np.zeros((nrows, nref), dtype=COUNTS)
    if nrows == 0:
        assert len(edges) == 0
        return out
    a = np.minimum(np.asarray(qn[q_begin:q_end], dtype=np.int64), s)
    b = np.minimum(np.asarray(rn[:nref], dtype=np.int64), s)
    out["denom"] = np.minimum(s, a[:, None] + b[None, :])
    if len(edges):
        row = edges["row"].astype(np.int64) - q_begin
        assert row.min() >= 0 and row.max() < nrows and int(edges["col"].max()) < nref
        out["numer"][row, edges["col"]] = edges["numer"]
        out["denom"][row, edges["col"]] = edges["denom"]
    return out


def edges_of(numer, denom, q_begin=0):
    """the exceptions of a dense [nq, nref] result: every pair with numer >= 1, query major, `row` offset by q_begin"""
    q, r = np.nonzero(numer >= 1)
    e = np.zeros(len(q), dtype=np.dtype([("row", "<u4"), ("col", "<u4"), ("numer", "<u4"), ("denom", "<u4")]))
    e["row"], e["col"], e["numer"], e["denom"] = q + q_begin, r, numer[q, r], denom[q, r]
    return e


def shares_a_hash(rt, rn, qt, qn, s):
    """bool [nq, nref]: the two sketches (each cut to its first min(nhash, s) hashes) have a hash in common"""
    nref = len(rn)
    cols = np.arange(min(rt.shape[1], s))[None, :]
    refs = np.where(cols < np.minimum(rn, s)[:, None], rt[:, :cols.shape[1]], PAD)
    out = np.zeros((len(qn), nref), dtype=bool)
    for q in range(len(qn)):
        mine = qt[q, : min(int(qn[q]), s)]
        if len(mine):
            out[q] = np.isin(refs, mine).any(axis=1)
    return out


def _pad_rows(table, nhash):
    table = table.copy()
    table[np.arange(table.shape[1])[None, :] >= nhash[:, None]] = PAD
    return table


def rect_case_clean():
    """1 200 references without an empty, short or copied row (the list engine takes the table) and 87 queries: copies of
    references, relatives, strangers, and the edges of the merge.  Returns a dict of the six arrays and what is where."""
    from workloads import synth
    nref, s = 1200, 256
    table, nhash, _ = synth.clustered_sketches(1240, s, clusters=24, seed=21, pool=400, private=100)
    rng = np.random.default_rng(8)
    rl = rng.integers(10 ** 4, 10 ** 8, nref).astype(np.uint64)
    rt, rn = table[:nref], nhash[:nref]
    spare_t, spare_n = table[nref:], nhash[nref:]
    originals = rng.choice(nref, 24, replace=False)
    st, sn, _ = synth.random_sketches(16, s, seed=5)
    rows, counts = [], []

    def add(h, n=None):
        row = np.full(s, PAD, dtype=np.uint64)
        n = len(h) if n is None else n
        row[:n] = h[:n]
        rows.append(row)
        counts.append(n)
        return len(rows) - 1

    for o in originals:
        add(rt[o], int(rn[o]))
    for i in range(40):
        add(spare_t[i], int(spare_n[i]))
    for i in range(16):
        add(st[i], int(sn[i]))
    where = {"copies": (0, originals), "relatives": 24, "strangers": 64}
    where["empty"] = add(np.zeros(0, dtype=np.uint64))
    where["last_of_7"] = add(rt[7, int(rn[7]) - 1: int(rn[7])])
    where["above"] = add(np.uint64(0xFFFFFFFFFFFFFF00) - np.arange(s, 0, -1, dtype=np.uint64))
    where["behind_11"] = add(np.concatenate([np.arange(1, s, dtype=np.uint64), rt[11, int(rn[11]) - 1: int(rn[11])]]))
    where["short"] = add(spare_t[3], 90)
    where["twice"] = (add(spare_t[5], int(spare_n[5])), add(spare_t[5], int(spare_n[5])))
    qt, qn = np.stack(rows), np.array(counts, dtype=np.uint32)
    ql = rng.integers(10 ** 4, 10 ** 8, len(qn)).astype(np.uint64)
    return {"rt": np.ascontiguousarray(rt), "rn": rn.copy(), "rl": rl, "qt": qt, "qn": qn, "ql": ql, "where": where}


def rect_case_ragged():
    """the references of rect_case_clean with short, empty and copied rows (the list engine declines such a table) and the 40
    spare rows as queries, every third one short and one empty"""
    from workloads import synth
    nref, s = 1200, 256
    table, nhash, _ = synth.clustered_sketches(1240, s, clusters=24, seed=21, pool=400, private=100)
    rng = np.random.default_rng(8)
    rl = rng.integers(10 ** 4, 10 ** 8, nref).astype(np.uint64)
    ql = rng.integers(10 ** 4, 10 ** 8, 40).astype(np.uint64)
    rt, rn = table[:nref].copy(), nhash[:nref].copy()
    qt, qn = table[nref:].copy(), nhash[nref:].copy()
    for i in range(0, nref, 7):
        rn[i] = rng.integers(0, 200)
    rn[3] = rn[4] = 0
    rn[9] = 1
    rn[10] = s - 1
    rt[21], rn[21] = rt[20], rn[20]
    for i in range(0, 40, 3):
        qn[i] = rng.integers(1, 150)
    qn[1] = 0
    return {"rt": _pad_rows(rt, rn), "rn": rn, "rl": rl, "qt": _pad_rows(qt, qn), "qn": qn, "ql": ql, "where": {}}


def rect_case_species():
    """600 rows of one species as references; 40 of them and 20 rows of another tree of descent as queries"""
    from workloads import synth
    rt, rn, rl = synth.species_sketches(600, 256, seed=9)
    ot, on, ol = synth.species_sketches(20, 256, seed=10)
    return {"rt": rt, "rn": rn, "rl": rl, "qt": np.concatenate([rt[100:140], ot]), "qn": np.concatenate([rn[100:140], on]),
            "ql": np.concatenate([rl[100:140], ol]), "where": {"own": (0, 40), "strangers": (40, 60)}}


def rect_case_sized(case, s_ref, s_qry):
    """the same arrays with the reference table cut to s_ref columns and the query table to s_qry (nhash clamped)"""
    out = dict(case)
    out["rt"] = np.ascontiguousarray(case["rt"][:, :s_ref])
    out["rn"] = np.minimum(case["rn"], s_ref).astype(np.uint32)
    out["qt"] = np.ascontiguousarray(case["qt"][:, :s_qry])
    out["qn"] = np.minimum(case["qn"], s_qry).astype(np.uint32)
    return out


def rect_case_oracle(oracle, case, k=21, kspace=4.0 ** 21):
    return rect_oracle(oracle, case["rt"], case["rn"], case["rl"], case["qt"], case["qn"], case["ql"], k, kspace)


def check_rect_case_conditions(name, case, numer, denom):
    """What the rect tests rely on, asserted on the oracle's output alone (the counts in the comments: what this seed gives)."""
    s = min(case["rt"].shape[1], case["qt"].shape[1])
    nq, nref = numer.shape
    w = case["where"]
    if name == "clean":
        assert (nq, nref) == (87, 1200)
        assert case["rn"].min() == 256 and case["qn"][:80].min() == 256                   # no short row among the references
        assert len(np.unique(case["rt"], axis=0)) == nref                                  # no copied row
        hit = numer >= 1
        assert 0.01 * numer.size < hit.sum() < 0.2 * numer.size                            # 3 382 of 104 400
        behind = shares_a_hash(case["rt"], case["rn"], case["qt"], case["qn"], s) & ~hit
        assert behind.sum() >= 1 and behind[w["behind_11"], 11]                            # 1: shares a hash, numer 0
        q0, originals = w["copies"]
        for i, o in enumerate(originals):                                                  # every copy finds its original
            assert numer[q0 + i, o] == case["rn"][o] == denom[q0 + i, o]
        assert not numer[w["strangers"]: w["strangers"] + 16].any() and not numer[w["empty"]].any() and not numer[w["above"]].any()
        assert np.array_equal(denom[w["empty"]], np.minimum(case["rn"], s))                # |A| + 0
        assert numer[w["last_of_7"], 7] == 1 and denom[w["last_of_7"], 7] == 256           # ... as the last union element
        assert numer[w["relatives"]: w["relatives"] + 40].max() > 100
        assert case["qn"][w["short"]] == 90 and numer[w["short"]].max() > 0
        a, b = w["twice"]
        assert np.array_equal(numer[a], numer[b]) and np.array_equal(denom[a], denom[b]) and numer[a].any()
    elif name == "ragged":
        assert (nq, nref) == (40, 1200)
        hit = numer >= 1
        assert len(np.unique(denom)) >= 100                                                # 255
        assert ((numer == 0) & (denom == 0)).sum() >= 1                                    # 2: empty against empty
        assert 0.01 * numer.size <= hit.sum() <= 0.2 * numer.size                          # 1 945 of 48 000
        assert np.array_equal(case["rt"][21], case["rt"][20]) and case["rn"][9] == 1 and case["rn"][10] == 255
    elif name == "species":
        assert (nq, nref) == (60, 600)
        (a, b), (c, d) = w["own"], w["strangers"]
        own = np.delete(numer[a:b], np.arange(100, 140), axis=1)                           # (without the rows themselves)
        assert 0.08 * 256 < np.percentile(own, 1) and np.percentile(own, 99) < 0.6 * 256   # 36 .. 106 of 256
        assert all(numer[i, 100 + i] == 256 for i in range(40))
        assert not numer[c:d].any()
    else:
        raise AssertionError(name)


# ---------------------------------------------------------------------------------------------- finished records against the oracle

def _set_kernel(monkeypatch, kernel):
    """tests/test_gpu_parity.py's conventions; "default": the dispatch's own choice"""
    for v in ("MASHGPU_COMPARE_KERNEL", "MASHGPU_COMPARE_WINDOWS", "MASHGPU_COMPARE_WIN_TARGET", "MASHGPU_RESULTS_MATRIX"):
        monkeypatch.delenv(v, raising=False)
    if kernel == "default":
        return
    if kernel == "plain":
        monkeypatch.setenv("MASHGPU_COMPARE_KERNEL", "merged")
        monkeypatch.setenv("MASHGPU_COMPARE_WINDOWS", "0")
    elif kernel.startswith("windows"):
        monkeypatch.setenv("MASHGPU_COMPARE_KERNEL", "merged")
        monkeypatch.setenv("MASHGPU_COMPARE_WINDOWS", "1")
        if kernel != "windows":
            monkeypatch.setenv("MASHGPU_COMPARE_WIN_TARGET", kernel[len("windows"):])
    else:
        monkeypatch.setenv("MASHGPU_COMPARE_KERNEL", kernel)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _oracle_pass(c, max_d, max_p):
    """compareSketches' two filters (CommandDistance.cpp:409-422) on the oracle's distances and p-values"""
    ok = np.ones(c["numer"].shape, dtype=bool)
    if max_d >= 0:
        ok &= c["dist"] <= max_d
    if max_p >= 0:
        ok &= c["pval"] <= max_p
    return ok


def _check_records_against_oracle(rec, c, lo, hi, max_d, max_p):
    """finished records against the oracle's arrays c["numer"], c["denom"], c["dist"], c["pval"] cut to [lo:hi) along their first
    axis -- queries [lo, hi) of a [nq, nref] rect result, or pairs [lo, hi) of a triangle's flat arrays: integers, pass and
    distance equal, p-values at the oracle's own accuracy (where the distance filter rejected a pair only `pass` is meaningful)"""
    assert np.array_equal(rec["numer"], c["numer"][lo:hi]) and np.array_equal(rec["denom"], c["denom"][lo:hi])
    assert np.array_equal(rec["pass"] == 1, _oracle_pass(c, max_d, max_p)[lo:hi])
    assert np.array_equal(rec["distance"], c["dist"][lo:hi])
    seen = c["dist"][lo:hi] <= max_d if max_d >= 0 else np.ones(rec.shape, dtype=bool)
    got, want = rec["p_value"][seen], c["pval"][lo:hi][seen]
    big = want > 1e-290
    assert np.all(np.abs(got[big] - want[big]) <= 1e-9 * want[big]) and np.all(got[~big] <= 1e-280)


# ---------------------------------------------------------------------------------------------- triangle jobs against the oracle
#
# The judge is oracle.triangle(table, nhash, lengths, rb, re, k, kspace, stats=True): flat arrays in reference order (row rb
# against rows 0 .. rb - 1, then row rb + 1, ...; row 0 has no pair).

EDGE = np.dtype([("row", "<u4"), ("col", "<u4"), ("numer", "<u4"), ("denom", "<u4")])        # mg_edge


def tri_base(row):
    """the pairs of the triangle ahead of `row`"""
    return row * (row - 1) // 2 if row > 0 else 0


def tri_slice(flat, rb, re):
    """the slice of a WHOLE triangle's flat array that rows [rb, re) occupy"""
    return flat[tri_base(rb): tri_base(max(re, rb))]


def tri_rows_cols(rb, re):
    """(row, col) of every pair of rows [rb, re), reference order"""
    r = np.arange(rb, max(re, rb), dtype=np.int64)
    rows = np.repeat(r, r)
    start = np.repeat(r * (r - 1) // 2 - tri_base(rb), r)               # where each pair's row begins in the range
    return rows, np.arange(len(rows), dtype=np.int64) - start


def edges_of_tri(numer, denom, rb, re):
    """the exceptions of rows [rb, re): every pair with numer >= 1 as {row, col, numer, denom} with table indices, reference order;
    numer and denom are the flat arrays OF THE RANGE (oracle.triangle over [rb, re), or tri_slice of the whole triangle)"""
    rows, cols = tri_rows_cols(rb, re)
    assert len(numer) == len(rows) == len(denom)
    at = np.nonzero(numer >= 1)[0]
    e = np.zeros(len(at), dtype=EDGE)
    e["row"], e["col"], e["numer"], e["denom"] = rows[at], cols[at], numer[at], denom[at]
    return e


def expand_tri(edges, nhash, s, rb, re):
    """The dense counts of rows [rb, re) out of mg_compare_tri_sparse_host's exceptions (include/mashgpu.h): every pair is
    {0, min(s, |A| + |B|)} with |X| = min(nhash, s), except the pairs listed in `edges`.  The CPU judge of mg_expand_tri_sparse."""
    re = min(re, len(nhash))
    rows, cols = tri_rows_cols(rb, re)
    out = np.zeros(len(rows), dtype=COUNTS)
    if len(rows) == 0:
        assert len(edges) == 0
        return out
    size = np.minimum(np.asarray(nhash, dtype=np.int64), s)
    out["denom"] = np.minimum(s, size[rows] + size[cols])
    if len(edges):
        r, c = edges["row"].astype(np.int64), edges["col"].astype(np.int64)
        assert r.min() >= rb and r.max() < re and np.all(c < r)
        at = r * (r - 1) // 2 - tri_base(rb) + c
        out["numer"][at] = edges["numer"]
        out["denom"][at] = edges["denom"]
    return out


def clade_table(rng, sizes, s, keep=0.96, private=0.03, short_every=0, gap_rows=3, short_min=1 / 3):
    """tests/test_gpu_parity.py's _clade_table (without its clumps): consecutive clades of the given sizes, near-copies of a pool
    of 1.06 s values, `gap_rows` unrelated rows behind each, every short_every-th row of a clade cut to short_min s .. s - 1
    hashes; returns (table, nhash, [(first, last + 1) of every clade])"""
    rows, spans = [], []
    for m in sizes:
        pool = np.unique(rng.integers(1, 1 << 60, size=int(1.06 * s) + 8).astype(np.uint64))
        spans.append((len(rows), len(rows) + m))
        for i in range(m):
            own = pool[rng.random(len(pool)) < keep]
            priv = rng.integers(1, 1 << 60, size=max(1, int(private * s))).astype(np.uint64)
            r = np.unique(np.concatenate([own, priv]))
            k = s if not (short_every and i % short_every == 1) else int(rng.integers(int(short_min * s), s))
            rows.append(r[:k])
        for _ in range(gap_rows):
            rows.append(np.unique(rng.integers(1, 1 << 60, size=s + 8).astype(np.uint64))[:s])
    table = np.full((len(rows), s), PAD, dtype=np.uint64)
    nhash = np.zeros(len(rows), dtype=np.uint32)
    for i, r in enumerate(rows):
        table[i, : len(r)] = r
        nhash[i] = len(r)
    return table, nhash, spans


def _tri_case(table, nhash, lengths, where):
    return {"table": np.ascontiguousarray(table), "nhash": np.ascontiguousarray(nhash, dtype=np.uint32),
            "lengths": np.ascontiguousarray(lengths, dtype=np.uint64), "n": len(nhash), "s": table.shape[1], "where": where}


def tri_case_families():
    """3 200 rows of s = 64 in 16 interleaved families, every third row with 20 .. 97 % of its hashes replaced: the smallest table
    on which a proper range of rows still has 4 * 10^6 pairs (the prefix view of host_compare.cpp engages).  No empty, short or
    copied row: the list engine takes the table.  Row 3001 shares its last hash with row 11 -- behind the 64 smallest of their
    union, so the pair counts nothing."""
    from workloads import synth
    n, s = 3200, 64
    table, nhash, _ = synth.clustered_sketches(n, s, clusters=16, seed=61, pool=80, private=8, keep_p=0.9)
    table, nhash = table.copy(), nhash.copy()
    rng = np.random.default_rng(3)
    for i in range(0, n, 3):
        u = rng.uniform(0.2, 0.97)
        m = rng.random(s) < u
        row = table[i].copy()
        row[m] = rng.integers(1, 1 << 60, int(m.sum())).astype(np.uint64)
        table[i] = np.sort(row)
    lengths = rng.integers(10 ** 4, 10 ** 8, n).astype(np.uint64)
    table[3001] = np.concatenate([np.arange(1, s, dtype=np.uint64), table[11, s - 1:]])
    return _tri_case(table, nhash, lengths, {"behind": (3001, 11)})


def tri_case_families_ragged():
    """tri_case_families with empty, short and copied rows: the list engine declines such a table, so list jobs take the blocked
    matrix path"""
    c = tri_case_families()
    table, nhash = c["table"].copy(), c["nhash"].copy()
    rng = np.random.default_rng(4)
    for i in range(0, c["n"], 50):
        nhash[i] = rng.integers(1, 64)
    nhash[100] = nhash[2950] = 0
    nhash[150], nhash[250] = 1, 63
    table[2000], nhash[2000] = table[1999], nhash[1999]
    table[3100], nhash[3100] = table[7], nhash[7]
    where = {"empty": (100, 2950), "copies": ((2000, 1999), (3100, 7)), "one_hash": 150, "one_short": 250}
    return _tri_case(_pad_rows(table, nhash), nhash, c["lengths"], where)


def tri_case_head(case, n):
    """the first n rows of a case as a case of its own"""
    return _tri_case(case["table"][:n], case["nhash"][:n], case["lengths"][:n], {})


def tri_case_clades():
    """520 rows of s = 128: six consecutive clades of near-copies, every fifth row of a clade short (103 .. 127 hashes), three unrelated rows behind each"""
    rng = np.random.default_rng(77)
    table, nhash, spans = clade_table(rng, (70, 9, 200, 33, 150, 40), 128, keep=0.95, private=0.03, short_every=5, short_min=0.8)
    lengths = rng.integers(10 ** 4, 10 ** 8, len(nhash)).astype(np.uint64)
    return _tri_case(table, nhash, lengths, {"clades": spans})


def tri_case_species():
    """the rect suite's table: 600 rows of one species"""
    from workloads import synth
    table, nhash, lengths = synth.species_sketches(600, 256, seed=9)
    return _tri_case(table, nhash, lengths, {})


def tri_case_oracle(oracle, case, k=21, kspace=4.0 ** 21):
    """the oracle's whole triangle of a case: (numer, denom, dist, pval), flat"""
    return oracle.triangle(case["table"], case["nhash"], case["lengths"], 0, case["n"], k, kspace, stats=True)


# What the GPU tests ask of a filter that is on: (max_d, max_p) and whether it may pass nothing
TRI_FILTERS_FAMILIES = ((0.05, -1.0), (0.03, -1.0), (-1.0, 1e-30), (0.05, 1e-30), (0.0, 1.0))


def check_tri_case_conditions(name, case, numer, denom, dist, pval):
    """What the triangle tests rely on, asserted on the oracle's output alone (the counts in the comments: what these seeds give)."""
    n, s, w = case["n"], case["s"], case["where"]
    assert len(numer) == n * (n - 1) // 2
    hit = numer >= 1
    if name == "families":
        assert case["table"].shape == (3200, 64) and case["nhash"].min() == 64               # no short row
        assert len(np.unique(case["table"], axis=0)) == n                                     # no copied row
        assert 0.01 * numer.size < hit.sum() < 0.2 * numer.size                               # 315 396 of 5 118 400 (6.2 %)
        row, col = w["behind"]
        assert case["table"][row, s - 1] == case["table"][col, s - 1]                         # shares a hash ...
        assert numer[tri_base(row) + col] == 0 and denom[tri_base(row) + col] == s            # ... and counts nothing
        c = {"numer": numer, "denom": denom, "dist": dist, "pval": pval}
        for max_d, max_p in TRI_FILTERS_FAMILIES:
            share = (_oracle_pass(c, max_d, max_p) & hit).sum() / hit.sum()
            if (max_d, max_p) == (0.0, 1.0):
                assert share == 0                                                             # nothing: no copy in the table
            else:
                assert 0.05 < share < 0.95, (max_d, max_p, share)                             # 78 %, 63 %, 89 %, 78 % of the hits
    elif name == "families_ragged":
        assert case["table"].shape == (3200, 64)
        # (a denominator at s = 64 is one of 0 .. 64: "at least 100 distinct" cannot hold on this table; nearly all of the 65 must)
        assert len(np.unique(denom)) >= 60                                                    # 62
        a, b = w["empty"]
        assert numer[tri_base(b) + a] == 0 and denom[tri_base(b) + a] == 0                    # empty against empty
        assert ((numer == 0) & (denom == 0)).sum() >= 1                                       # 1
        for row, col in w["copies"]:
            assert numer[tri_base(row) + col] == denom[tri_base(row) + col] == case["nhash"][row] == case["nhash"][col]
        assert case["nhash"][w["one_hash"]] == 1 and case["nhash"][w["one_short"]] == 63
        assert 0.01 * numer.size < hit.sum() < 0.2 * numer.size                               # 314 855 (6.2 %)
    elif name == "clades":
        assert 500 <= n <= 540 and s == 128
        rows, cols = tri_rows_cols(0, n)
        for a, b in w["clades"]:
            inside = (rows >= a) & (rows < b) & (cols >= a)
            assert np.percentile(numer[inside], 1) > 0.5 * s, (a, b)                          # 92 .. 101 of 128
        assert (case["nhash"] < s).sum() >= 50 and (numer == 0).any()                           # 101 short rows; 74 % of the pairs
    elif name == "species":
        assert (n, s) == (600, 256)
        assert 0.08 * s < np.percentile(numer, 1) and np.percentile(numer, 99) < 0.6 * s      # 37 .. 102 of 256
    else:
        raise AssertionError(name)


# ---------------------------------------------------------------------------------------------- screen probes against the oracle
#
# `mash screen` counts, for every hash of every database row, how often the mixture holds a k-mer of that hash.  The judge hashes
# every valid k-mer of the mixture with the oracle and counts; the cases below steer the fused sketch + probe kernel onto the
# paths that exist to keep a k-mer from being counted twice (a steady tile that overflows the candidate buffer, a seeded batch
# that comes out short and is run again).  tests/test_screen_probe_oracle.py asserts, on the oracle's output alone, that they do.

SCREEN_PROTEIN = "ACDEFGHIKLMNPQRSTVWY"
RECORD_SEP = b"\n"                                                         # MG_RECORD_SEP (include/mashgpu.h)


def _all_kmer_hashes(oracle, records, p):
    bases = np.frombuffer(b"".join(records), dtype=np.uint8).copy()       # (the oracle upper-cases in place)
    off = np.zeros(len(records) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in records], dtype=np.uint64)
    return oracle.kmer_hashes(bases, off, p).copy()


def screen_batch_hashes(oracle, params_kw, records, translate=False):
    """the hash of every valid k-mer of one batch, occurrences repeated (translate: of every frame of six_frames(record))"""
    if translate:
        records = [fr for r in records for fr in oracle.six_frames(r)]
    return _all_kmer_hashes(oracle, records, oracle.params(**params_kw))


def screen_expected(oracle, params_kw, batches, translate=False):
    """What a screen of the mixture `batches` (lists of records) must report, by the oracle alone:
    (counts: dict hash -> occurrences over every record of every batch, mix: u64[<= s], the s smallest distinct hashes)."""
    parts = [screen_batch_hashes(oracle, params_kw, recs, translate) for recs in batches]
    allh = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint64)
    u, c = np.unique(allh, return_counts=True)
    return dict(zip(u.tolist(), c.tolist())), u[: params_kw.get("s", 1000)].copy()


def screen_expected_rows(counts, table, nhash):
    """the dense u32[n, s] result of the database (table, nhash) out of screen_expected's dict: zero behind a row's nhash"""
    out = np.zeros(table.shape, dtype=np.uint32)
    for i in range(table.shape[0]):
        out[i, : nhash[i]] = [counts.get(h, 0) for h in table[i, : nhash[i]].tolist()]
    return out


def hits_equal_counts(hits, counts, table, nhash):
    """tests/test_gpu_parity.py's _hits_equal_counts: hits == the non-zero cells of the dense counts matrix, hash values included,
    ordered by row then hash"""
    from mash_amd import abi
    r, c = np.nonzero(counts)
    assert len(hits) == len(r)
    want = np.zeros(len(r), dtype=abi.HIT_DTYPE)
    want["row"], want["count"], want["hash"] = r, counts[r, c], table[r, c]
    want = want[np.lexsort((want["hash"], want["row"]))]
    assert np.array_equal(hits, want)


def screen_db(oracle, case):
    """the database of a case, sketched by the oracle: (table u64[n, s] padded, nhash u32[n], lengths u64[n])"""
    kw = case["params"]
    s = kw["s"]
    p = oracle.params(**kw)
    table = np.full((len(case["db"]), s), PAD, dtype=np.uint64)
    nhash = np.zeros(len(case["db"]), dtype=np.uint32)
    for i, recs in enumerate(case["db"]):
        if i in case.get("db_six_frames", ()):                            # a nucleotide row of an amino-acid database
            recs = [fr for r in recs for fr in oracle.six_frames(r)]
        h = oracle.sketch_records(list(recs), p)[0]
        table[i, : len(h)] = h
        nhash[i] = len(h)
    lengths = np.array([max(sum(len(r) for r in recs), 1) for recs in case["db"]], dtype=np.uint64)
    return table, nhash, lengths


def screen_blob(records):
    """one batch as mg_screen_add_host takes it: the records joined with the separator"""
    return np.frombuffer(RECORD_SEP.join(records), dtype=np.uint8)


def screen_batch_npos(case, records):
    """the k-mer starts the sketch kernel sees in one batch -- what seed_thresholds (host_sketch.cpp) calls npos: the joined bytes
    are one sketch; a translated batch is six frames of nbases / 3 + 1 bytes each, rounded up to 16 (screen_add_translated,
    host_screen.cpp)"""
    nbases = len(RECORD_SEP.join(records))
    if case["translate"]:
        nbases = 6 * ((nbases // 3 + 1 + 15) & ~15)
    return nbases - case["params"]["k"] + 1


def _revcomp(b):
    return bytes({65: 84, 67: 71, 71: 67, 84: 65, 78: 78}[x] for x in reversed(b))


def _screen_reads(rng, genomes, n, lo=120, hi=150, fresh=2 / 3, revcomp=True):
    """n reads of lo .. hi bases: `fresh` of them random sequence of their own, the others cut out of `genomes`; some with an N,
    some lower case, half of them reverse complements.  (The fresh ones keep a batch's distinct k-mers above a third of its
    k-mer starts: a batch of genome reads and a 10^5-base run alone comes out short of its seeded threshold and is run again.)"""
    from workloads import synth
    out = []
    for _ in range(n):
        l = int(rng.integers(lo, hi + 1))
        if rng.random() < fresh:
            r = bytearray(synth._rand_dna(rng, l))
        else:
            g = genomes[int(rng.integers(0, len(genomes)))]
            st = int(rng.integers(0, len(g) - l))
            r = bytearray(g[st:st + l])
        u = rng.random()
        if u < 0.2:
            r[int(rng.integers(0, l))] = ord("N")
        elif u < 0.35:
            r = bytearray(bytes(r).lower())
        out.append(bytes(r) if not revcomp or rng.random() < 0.5 else _revcomp(bytes(r).upper()))
    return out


def _screen_dna_parts():
    """what every DNA case shares: four 30 kbp genomes (the last is never sampled) and the two repeat units"""
    from workloads import synth
    rng = np.random.default_rng(2024)
    genomes = [synth._rand_dna(rng, 30000) for _ in range(4)]
    return genomes, synth._rand_dna(rng, 700), synth._rand_dna(rng, 2500), synth._rand_dna(rng, 23)


def _screen_dna_db(k):
    """rows 0, 1: one hash, twice (rows that share a key each get their hit); row 2: the T run's hash (the same key when k-mers
    are canonical); rows 3 .. 5: the genomes the reads come from; row 6: a genome never sampled; rows 7, 8: the two repeat units
    with the k-mers across their seam (ragged rows where the unit has fewer than s distinct k-mers)"""
    genomes, unit_small, unit_mid, _ = _screen_dna_parts()
    return [[b"A" * 100], [b"A" * 100], [b"T" * 100]] + [[g] for g in genomes] + [[unit_small + unit_small[: k - 1]], [unit_mid + unit_mid[: k - 1]]]


SCREEN_DNA_UNSAMPLED = (6,)

# Hash seeds found by a search with the oracle (get_hash over seeds 1, 2, ...); test_screen_probe_oracle.py checks what they are for
SCREEN_SEED_FLOOD = 6713            # hash64("A" * 21) at 7.4e-6 of the range
SCREEN_SEED_FORWARD = 1490799       # hash32("A" * 16) at 8.8e-4 and hash32("T" * 16) at 7.0e-4 of the 32-bit range
SCREEN_SEED_TRANSLATED = 87512      # hash32("K" * 7) at 3.4e-6 of the 32-bit range


def _flood_batches(rng, genomes, unit23):
    from workloads import synth
    long_record = synth._rand_dna(rng, 3000) + b"A" * 50000 + synth._rand_dna(rng, 2000) + unit23 * 4000 + b"T" * 50000
    one = _screen_reads(rng, genomes[:3], 1500) + [long_record] + _screen_reads(rng, genomes[:3], 500)
    return [one, _screen_reads(rng, genomes[:3], 1500)]


def screen_case_flood(s=1000):
    """canonical 21-mers: 2 000 reads around one record with a run of 50 000 A, 4 000 copies of a 23-mer and a run of 50 000 T
    (the A run's canonical key again); a second batch of reads only"""
    genomes, _, _, unit23 = _screen_dna_parts()
    rng = np.random.default_rng(301)
    return {"params": {"k": 21, "s": s, "seed": SCREEN_SEED_FLOOD}, "translate": False, "db": _screen_dna_db(21),
            "batches": _flood_batches(rng, genomes, unit23), "runs": [(0, b"A" * 21, 50000 - 20), (0, b"T" * 21, 50000 - 20)],
            "short": {}, "hot": 10000, "unsampled": SCREEN_DNA_UNSAMPLED}


def screen_case_flood_wide():
    """screen_case_flood at s = 3000: the NT = 1024 kernels, tiles of 28 672; the runs are 100 000 long"""
    from workloads import synth
    genomes, _, _, unit23 = _screen_dna_parts()
    rng = np.random.default_rng(302)
    long_record = synth._rand_dna(rng, 3000) + b"A" * 100000 + synth._rand_dna(rng, 2000) + unit23 * 4000 + b"T" * 100000
    one = _screen_reads(rng, genomes[:3], 2500) + [long_record] + _screen_reads(rng, genomes[:3], 1000)
    return {"params": {"k": 21, "s": 3000, "seed": SCREEN_SEED_FLOOD}, "translate": False, "db": _screen_dna_db(21),
            "batches": [one, _screen_reads(rng, genomes[:3], 1500)], "runs": [(0, b"A" * 21, 100000 - 20), (0, b"T" * 21, 100000 - 20)],
            "short": {}, "hot": 10000, "unsampled": SCREEN_DNA_UNSAMPLED}


def screen_case_flood_forward():
    """forward-only 16-mers (MODE 1, 32-bit hashes): the A run and the T run are different keys"""
    genomes, _, _, unit23 = _screen_dna_parts()
    rng = np.random.default_rng(303)
    return {"params": {"k": 16, "s": 1000, "seed": SCREEN_SEED_FORWARD, "noncanonical": True}, "translate": False, "db": _screen_dna_db(16),
            "batches": _flood_batches(rng, genomes, unit23), "runs": [(0, b"A" * 16, 50000 - 15), (0, b"T" * 16, 50000 - 15)],
            "short": {}, "hot": 10000, "unsampled": SCREEN_DNA_UNSAMPLED}


def screen_case_flood_translated():
    """amino-acid 7-mers against a nucleotide mixture translated in six frames: 150 000 A give a run of 50 000 K in each forward
    frame.  Rows 0 .. 2: the six frames of three 9 kbp genomes (the last never sampled, but random sequence meets some of its
    7-mers by chance); rows 3, 4: the sketch of K * 50, twice; row 5: a peptide of M and W, one codon each, which random
    sequence does not meet (a ragged row: at most 2^7 k-mers)."""
    from workloads import synth
    rng = np.random.default_rng(304)
    genomes = [synth._rand_dna(rng, 9000) for _ in range(3)]
    rare = np.frombuffer(b"MW", dtype=np.uint8)[rng.integers(0, 2, 400)].tobytes()
    reads = lambda n: _screen_reads(rng, genomes[:2], n, lo=150, hi=300, fresh=3 / 4)
    one = reads(1200) + [b"AC", b"A" * 150000, b""] + reads(700)
    return {"params": {"k": 7, "s": 300, "seed": SCREEN_SEED_TRANSLATED, "alphabet": SCREEN_PROTEIN, "noncanonical": True}, "translate": True,
            "db": [[g] for g in genomes] + [[b"K" * 50], [b"K" * 50], [rare]], "db_six_frames": (0, 1, 2),
            "batches": [one, reads(600)], "runs": [(0, b"K" * 7, 50000 - 6)], "short": {}, "hot": 10000, "unsampled": (5,)}


def screen_case_short():
    """canonical 21-mers, three batches: 400 copies of a 700-base unit (fewer than s distinct k-mers), 120 copies of a 2 500-base
    unit (s distinct k-mers, but next to none below the seeded threshold), ordinary reads"""
    genomes, unit_small, unit_mid, _ = _screen_dna_parts()
    rng = np.random.default_rng(305)
    return {"params": {"k": 21, "s": 1000, "seed": SCREEN_SEED_FLOOD}, "translate": False, "db": _screen_dna_db(21),
            "batches": [[unit_small * 400], [unit_mid * 120], _screen_reads(rng, genomes[:3], 1500)], "runs": [],
            "short": {0: "a", 1: "b"}, "hot": 100, "unsampled": SCREEN_DNA_UNSAMPLED}


def screen_case_batch_edges():
    """canonical 21-mers, batches at the edges of the batch format: shorter than k, exactly k bytes (one k-mer, a database key),
    k bytes with a separator among them (one k-mer start, no k-mer), separators first and last, empty records, nothing but
    separators"""
    genomes, _, _, _ = _screen_dna_parts()
    rng = np.random.default_rng(306)
    r = lambda n: _screen_reads(rng, genomes[:3], n, fresh=0.0)
    return {"params": {"k": 21, "s": 1000, "seed": SCREEN_SEED_FLOOD}, "translate": False, "db": _screen_dna_db(21),
            "batches": [[b"ACGTACGTAC"], [b"A" * 21], [b"A" * 10, b"C" * 10], [b""] + r(40) + [b""], r(3) + [b"", b""] + r(20) + [b""] + r(7),
                        [b"", b"", b""], [b"", b"", genomes[0][500:521], b"", b""]],
            "runs": [], "short": {}, "hot": None, "unsampled": SCREEN_DNA_UNSAMPLED}


SCREEN_CASES = ("flood", "flood_wide", "flood_forward", "flood_translated", "short", "batch_edges")


def screen_case(name):
    return globals()["screen_case_" + name]()


# ---------------------------------------------------------------------------------------------- sketch kernels against the oracle
#
# tests/test_sketch_instances_gpu.py runs the sketch kernels (sketch.hip) at every instantiation, tile seam and merge level on the
# inputs built here; tests/test_sketch_cases_oracle.py asserts on the CPU that the inputs reach what they are built for.  The judge
# is oracle.sketch_records / oracle.sketch_reads, every comparison exact.
#
# The constants below RESTATE the engine's plan (plan_sketch_work, host_sketch.cpp; sketch_geometry, sketch.hip).  They are compared
# with nothing at run time: they are the tests' claim about the code, and a change of the plan is made in both places on purpose.

SKETCH_TILE = {256: 256 * 60, 1024: 1024 * 28}            # k-mer starts per tile: NT lanes of sk_L(NT) starts (kmer_stream.h)
SKETCH_MIN_CHUNK_TILES = 4                                # a chunk (one workgroup) is at least four tiles ...
SKETCH_TARGET_ITEMS = 2048                                # ... and a batch is cut into about this many
SKETCH_MERGE_GROUP = 32                                   # above 2 * 32 chunks a sketch is merged in groups of 32, then the groups
SKETCH_SEGMENT = {256: 256 * 4 * 2, 1024: 1024 * 4 * 1}   # candidates one segment may append: NT * 4 * sk_seg_dw(NT)
SKETCH_PER_LANE = 16                                      # the candidate buffer holds at most 16 hashes per lane (SK_E)
SKETCH_ONE_TILE = {"MASHGPU_SKETCH_MIN_CHUNK": "15360", "MASHGPU_SKETCH_ITEMS": "100000"}     # chunks of one tile (15 360 is rounded up)
SKETCH_ENV = ("MASHGPU_SKETCH_MIN_CHUNK", "MASHGPU_SKETCH_ITEMS", "MASHGPU_SKETCH_NO_SEED", "MASHGPU_SKETCH_SEED_FACTOR")
# MODE 0: canonical DNA, 1: forward-only DNA, 2: a table alphabet, forward-only
SKETCH_MODES = ({}, {"noncanonical": True}, {"alphabet": SCREEN_PROTEIN, "noncanonical": True})
_PROTEIN_LETTERS = np.frombuffer(SCREEN_PROTEIN.encode(), dtype=np.uint8)


def sketch_geometry(s):
    """(NT, capacity of the candidate buffer) the LDS selector takes for sketch size s, None where s goes to range counting in HBM:
    the capacity is the power of two that holds s and one segment, at most 16 hashes per lane"""
    for nt in (256, 1024):
        cap = 2
        while cap < s + SKETCH_SEGMENT[nt]:
            cap <<= 1
        if cap <= SKETCH_PER_LANE * nt:
            return nt, cap
    return None


def sketch_plan(lengths, k, nt, env=None):
    """plan_sketch_work restated: per sketch of the batch None (no k-mer) or {"chunks", "groups": slots per first-level merge ([]:
    one level), "last": k-mer starts of the last chunk}; env: the two knobs of the plan as the environment gives them"""
    env = env or {}
    tile = SKETCH_TILE[nt]
    total = sum(l - k + 1 for l in lengths if l >= k)
    items = max(int(env.get("MASHGPU_SKETCH_ITEMS", SKETCH_TARGET_ITEMS)), 1)
    chunk = max(-(-total // items), int(env.get("MASHGPU_SKETCH_MIN_CHUNK", SKETCH_MIN_CHUNK_TILES * tile)))
    chunk = -(-chunk // tile) * tile
    out = []
    for l in lengths:
        if l < k:
            out.append(None)
            continue
        npos = l - k + 1
        nch = -(-npos // chunk)
        g = SKETCH_MERGE_GROUP
        groups = [min(g, nch - i) for i in range(0, nch, g)] if nch > 2 * g else []
        out.append({"chunks": nch, "groups": groups, "last": npos - (nch - 1) * chunk})
    return out


def sketch_batch(blobs):
    """(bases u8[], off u64[n + 1]) of a batch as mg_sketch_host takes it: one blob (records joined with the separator) per sketch"""
    off = np.zeros(len(blobs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(b) for b in blobs], dtype=np.uint64)
    return np.frombuffer(b"".join(blobs), dtype=np.uint8), off


def sketch_expected(oracle, kw, bases, off):
    """the oracle's (hashes, counts) of every sketch of a batch: bytes [off[i], off[i + 1]) alone, cut into records at the separators"""
    p = oracle.params(**kw)
    raw = bases.tobytes()
    out = []
    for i in range(len(off) - 1):
        h, c, _, _, _ = oracle.sketch_records(raw[int(off[i]): int(off[i + 1])].split(RECORD_SEP), p)
        out.append((h, c))
    return out


def _rand_protein(rng, n):
    return _PROTEIN_LETTERS[rng.integers(0, 20, n)].tobytes()


# ---- 1. the wide selector (NT = 1024) at every k and mode

SKETCH_WIDE_SIZES = (2049, 4097, 12288)                    # the first s of NT = 1024, the first of capacity 16 384, the last of the selector


def sketch_case_wide(k):
    """{"s", "dna": sketches for MODE 0 and 1, "protein": sketches for MODE 2}; sketch 0 of each is one long record with two seams of
    the 28 672 tile (70 kbp) resp. one (40 000 residues where s = 12 288, which 12 000 residues cannot fill), the others adversarial"""
    from workloads import synth
    rng = np.random.default_rng(8100 + k)
    s = SKETCH_WIDE_SIZES[k % 3]
    dna = [[synth._rand_dna(rng, 70000)], synth.adversarial_dna_records(rng, 1), synth.adversarial_dna_records(rng, 2)]
    protein = [[_rand_protein(rng, 40000 if s == 12288 else 12000)], synth.random_protein_records(rng, 1)]
    return {"s": s, "dna": dna, "protein": protein}


# ---- 2. the boundaries of sketch_geometry

SKETCH_GEOMETRY_SIZES = {2048: (256, 4096), 2049: (1024, 8192), 4096: (1024, 8192), 4097: (1024, 16384), 12288: (1024, 16384), 12289: None}


def sketch_case_geometry():
    """{"dna": (kw, sketches), "protein": (kw, sketches)}: one record of 150 kbp at k = 21 canonical, one of 40 000 residues at k = 9"""
    from workloads import synth
    rng = np.random.default_rng(8200)
    return {"dna": ({"k": 21}, [[synth._rand_dna(rng, 150000)]]),
            "protein": (dict(SKETCH_MODES[2], k=9), [[_rand_protein(rng, 40000)]])}


# ---- 3. the event kernel (reads mode with -c / -b) at every k and mode

SKETCH_EVENT_READS, SKETCH_EVENT_COV, SKETCH_EVENT_BLOOM = 800, 3.0, 700


def sketch_case_events(k, mode):
    """800 reads of 40 .. 119 symbols cut out of a 3 000-symbol source (DNA: half of them reverse complements), every tenth with an
    invalid symbol"""
    from workloads import synth
    rng = np.random.default_rng(8300 + 3 * k + mode)
    src = _rand_protein(rng, 3000) if mode == 2 else synth._rand_dna(rng, 3000)
    reads = []
    for i in range(SKETCH_EVENT_READS):
        l = int(rng.integers(40, 120))
        st = int(rng.integers(0, 3000 - l))
        r = bytearray(src[st:st + l])
        if i % 10 == 9:
            r[int(rng.integers(0, l))] = ord("X" if mode == 2 else "N")
        r = bytes(r)
        reads.append(_revcomp(r) if mode != 2 and rng.random() < 0.5 else r)
    return reads


# ---- 4. an invalid byte and a record separator at every offset around a tile seam

SKETCH_SEAM_KS = (1, 4, 5, 16, 17, 21, 32)
SKETCH_SEAM_SIZES = (300, 3000)                            # NT = 256 and NT = 1024
SKETCH_SEAM_MODES = (5, 21)                                # the k-mer sizes that also run MODE 1 and MODE 2


def sketch_case_seams(k, s, mode=0):
    """(kw, bases, off, where): for every d in [-k, k] one sketch whose byte TILE + d is invalid (MODE 0: N; MODE 1 with preserve_case:
    a lower-case base; MODE 2: X) and one whose byte TILE + d is the record separator -- two records split there.  Every sketch is
    two tiles and 1 001 bytes long, an odd length of 9 mod 16, so that consecutive sketches begin at every alignment of the 16-byte
    loads; the sweep is repeated until the batch has 16 sketches.  where: (offset of the byte within its sketch, the byte) per sketch"""
    from workloads import synth
    nt, _ = sketch_geometry(s)
    tile = SKETCH_TILE[nt]
    rng = np.random.default_rng(8400 + 10 * k + mode + s)
    kw = dict(SKETCH_MODES[mode], k=k, s=s)
    if mode == 1:
        kw["preserve_case"] = True
    blobs, where = [], []
    while len(blobs) < 16:
        for d in range(-k, k + 1):
            for sep in (False, True):
                n = 2 * tile + 1001
                b = bytearray(_rand_protein(rng, n) if mode == 2 else synth._rand_dna(rng, n))
                at = tile + d
                b[at] = RECORD_SEP[0] if sep else (ord("N"), b[at] + 32, ord("X"))[mode]
                blobs.append(bytes(b))
                where.append((at, b[at]))
    bases, off = sketch_batch(blobs)
    return kw, bases, off, where


# ---- 5. slices of one genome: sketches that touch without a separator

SKETCH_SLICE_KS = (5, 16, 21, 32)


def sketch_slice_lengths(k, tile):
    return [0, k - 1, k, k + 1, 15, 16, 17, tile - 1, tile, tile + 1, tile + k - 2, tile + k - 1, tile + k,
            SKETCH_MIN_CHUNK_TILES * tile + k - 1,          # the largest sketch of one chunk
            SKETCH_MIN_CHUNK_TILES * tile + k]              # two chunks, the second of one k-mer start


def sketch_case_slices(k, s):
    """(kw, bases, off): one buffer of ACGT (about 400 kbp at the 28 672 tile) with three N in it, cut by off[] alone into slices of
    sketch_slice_lengths: a k-mer across a cut belongs to no sketch"""
    from workloads import synth
    nt, _ = sketch_geometry(s)
    lengths = sketch_slice_lengths(k, SKETCH_TILE[nt])
    off = np.zeros(len(lengths) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lengths, dtype=np.uint64)
    bases = synth.synthetic_genome(50 + k, int(off[-1])).copy()
    for i in (8, 12, 14):                                   # inside the slices of T, T + k and 4 T + k bytes
        bases[int(off[i]) + lengths[i] // 3] = ord("N")
    return {"k": k, "s": s}, bases, off


# ---- 6. the two-level merge

SKETCH_MERGE_CASES = {256: {"k": 21, "s": 1000}, 1024: {"k": 21, "s": 3000}}


def sketch_case_merge(nt):
    """(kw, bases, off, names) for chunks of one tile (SKETCH_ONE_TILE): sketches of exactly 64 chunks (one level), of 65 (groups of
    32, 32 and 1; the last chunk is one k-mer start), of 72 (a ragged last group), 72 chunks of a 700-base unit repeated (seeded,
    short, run again through both levels) and an ordinary one of 60 kbp"""
    from workloads import synth
    kw = dict(SKETCH_MERGE_CASES[nt])
    k, tile = kw["k"], SKETCH_TILE[nt]
    rng = np.random.default_rng(8600 + nt)
    unit = synth._rand_dna(rng, 700)
    blobs = {"c64": synth._rand_dna(rng, 64 * tile + k - 1), "c65": synth._rand_dna(rng, 64 * tile + k),
             "c72": synth._rand_dna(rng, 71 * tile + 5000 + k - 1), "repeat": (unit * (72 * tile // 700 + 1))[: 72 * tile],
             "plain": synth._rand_dna(rng, 60000)}
    bases, off = sketch_batch(list(blobs.values()))
    return kw, bases, off, list(blobs)


def sketch_case_merge_reads(nt=256):
    """(kw, reads): the 72-chunk genome of sketch_case_merge as reads of 5 000 bases that begin every 2 500: every base but the
    first and the last 2 500 is covered twice (min_copies = 2).  (In the order of the genome: the oracle's set of hashes seen once
    stays small, it is a sorted array.)"""
    kw, bases, off, names = sketch_case_merge(nt)
    i = names.index("c72")
    g = bases[int(off[i]): int(off[i + 1])].tobytes()
    return dict(kw, min_copies=2), [g[o:o + 5000] for o in range(0, len(g) - 2500, 2500)]


def sketch_case_genome():
    """(kw, record): a lone genome of 5 Mbp at the default plan, k = 21, s = 1 000 -- what `mash sketch` of one bacterial genome is"""
    from workloads import synth
    return {"k": 21, "s": 1000}, synth.synthetic_genome(77, 5_000_000).tobytes()
