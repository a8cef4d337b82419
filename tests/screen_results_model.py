"""Pure-Python model of the tail of `mash screen` (CommandScreen.cpp:331-455): the specification the GPU tests of
mg_screen_results_host are judged by.

Input: the hits of a mixture -- (row, count, hash) for every database row that holds a hash the mixture showed at least
once, count = how often -- with the rows' hash counts (`nhash`, the reference's hashesSorted.size()) and lengths.
Output: one record per line the command prints, (row, shared, denom, median, identity, p_value), in row order.

  shared   hits of the row (minCov is 1, :235, :338-355)
  winner   (-w, :357-407) score of a row = identity(shared, denom, k); every observed hash goes to ONE holder: highest
           score, then larger length, then LOWEST ROW.  The reference walks an unordered_set of holders, so its pick among
           holders of equal score and length is whatever that set's order gives; the model (and the library) fix it.
  median   sorted counts at index shared // 2, 0 when shared == 0 (:409-414, :436)
  identity 1.0 when shared == denom, 0.0 when shared == 0, else (shared / denom) ** (1 / k) -- Python's float power is the
           C library's pow, which is what estimateIdentity (:463-482) calls
  p_value  pValueWithin (:601-615).  The CPU oracle has no containment p-value; the model takes it from the exported host
           function mg_p_value_within, pinned by tests/test_pvalue_exact.py and the existing screen goldens.
  filters  a row is printed when (shared != 0 or min_identity < 0) and identity >= min_identity and p <= max_p (:420-434)

The model never calls the function under test."""
import collections
import os

PROTEIN = "ACDEFGHIKLMNPQRSTVWY"


def identity(x, d, k):
    if x == d:
        return 1.0
    if x == 0:
        return 0.0
    return (x / d) ** (1.0 / k)


def set_size(mix, bits=64):
    """estimateSetSize of the mixture's bottom-s sketch (MinHashHeap.h:45): mix = its hashes, ascending"""
    if len(mix) == 0:
        return 0
    return int(2.0 ** bits * float(len(mix)) / float(int(mix[-1])))


_LIB = None


def host_p_value_within(x, ssize, kmer_space, denom):
    global _LIB
    if _LIB is None:
        from mash_amd import abi
        _LIB = abi.load_library()
    return float(_LIB.mg_p_value_within(int(x), int(ssize), float(kmer_space), int(denom)))


def results(hits, nhash, lengths, k, ssize, kmer_space, winner=False, min_identity=0.0, max_p=1.0, p_value=host_p_value_within):
    """-> [(row, shared, denom, median, identity, p_value)] in row order"""
    n = len(nhash)
    depths = [[] for _ in range(n)]
    for row, count, _ in hits:
        depths[row].append(int(count))
    if winner:
        scores = [identity(len(depths[i]), int(nhash[i]), k) for i in range(n)]
        holders, obs = collections.defaultdict(list), {}
        for row, count, h in hits:
            holders[int(h)].append(int(row))
            obs[int(h)] = int(count)
        depths = [[] for _ in range(n)]
        for h, rows in holders.items():
            best = max(rows, key=lambda r: (scores[r], int(lengths[r]), -r))
            depths[best].append(obs[h])
    out = []
    for i in range(n):
        shared, denom = len(depths[i]), int(nhash[i])
        if shared == 0 and not min_identity < 0.0:
            continue
        ident = identity(shared, denom, k)
        if ident < min_identity:
            continue
        pv = 1.0 if shared == 0 else p_value(shared, ssize, kmer_space, denom)
        if pv > max_p:
            continue
        out.append((i, shared, denom, sorted(depths[i])[shared // 2] if shared else 0, ident, pv))
    return out


def hits_of(rows, observed):
    """rows: per database row its hashes; observed: {hash: observations} -> [(row, count, hash)] by row, then hash"""
    out = []
    for i, hashes in enumerate(rows):
        for h in sorted(int(x) for x in hashes):
            c = observed.get(h, 0)
            if c:
                out.append((i, c, h))
    return out


def lines(recs, names, comments):
    """the bytes `mash screen` prints (operator<< of a double is %g with six digits)"""
    return "".join("%g\t%d/%d\t%d\t%g\t%s\t%s\n" % (ident, shared, denom, med, pv, names[row], comments[row])
                   for row, shared, denom, med, ident, pv in recs).encode()


# -------------------------------------------------------------------------------------------------- file helpers
def fixture_inputs(orc, case, indir):
    """For a case of tests/golden/screen_results/cases.json: (names, comments, lengths, rows, observed {hash: count},
    mixture sketch) -- the database records with their bottom-s hashes and the k-mer hashes of the pool with their
    multiplicities, all from the CPU oracle"""
    import numpy as np
    from taxscreen_model import read_fastx
    aa = bool(case.get("protein"))
    k, s = case["k"], case["s"]
    p = orc.params(k=k, s=s, alphabet=PROTEIN if aa else "ACGT", noncanonical=aa)
    recs = []
    for db in case["db"]:
        recs += read_fastx(os.path.join(indir, db))
    rows = [orc.sketch_records([seq], p)[0] for _, _, seq in recs]
    observed = collections.Counter()
    for pool in case["pools"]:
        for _, _, seq in read_fastx(os.path.join(indir, pool)):
            if len(seq) < k:
                continue
            for part in (orc.six_frames(seq) if aa else [seq]):
                if len(part) < k:
                    continue
                b = np.frombuffer(bytes(part), dtype=np.uint8).copy()
                observed.update(int(x) for x in orc.kmer_hashes(b, np.array([0, len(b)], dtype=np.uint64), p))
    mix = sorted(observed)[:s]
    return [r[0] for r in recs], [r[1] for r in recs], [len(r[2]) for r in recs], rows, observed, mix


def case_options(case):
    """(winner, min_identity, max_p) of a case's command line"""
    cmd, winner, mi, mp = case["cmd"], False, 0.0, 1.0
    for i, a in enumerate(cmd):
        if a == "-w":
            winner = True
        elif a == "-i":
            mi = float(cmd[i + 1])
        elif a == "-v":
            mp = float(cmd[i + 1])
    return winner, mi, mp


def case_lines(orc, case, indir):
    names, comments, lengths, rows, observed, mix = fixture_inputs(orc, case, indir)
    aa = bool(case.get("protein"))
    winner, mi, mp = case_options(case)
    kmer_space = float(20 if aa else 4) ** case["k"]
    recs = results(hits_of(rows, observed), [len(r) for r in rows], lengths, case["k"], set_size(mix, 64 if kmer_space > 2.0 ** 32 else 32), kmer_space,
                   winner=winner, min_identity=mi, max_p=mp)
    return lines(recs, names, comments)
