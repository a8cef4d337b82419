"""mg_screen_results_host and the `mash screen` that prints from it, on the GPU, judged by tests/screen_results_model.py and
by the recorded stdout of the reference CLI (tests/golden/screen_results; tests/test_screen_results_model.py shows on the CPU
that the two agree on every parity fixture).  Through the command: every parity fixture byte for byte and the model's bytes
for the full tie, by the device route and by the host route (MASH_AMD_HOST_SCREEN_FINISH=1), with equal stderr.  Through
the C ABI: records equal the model field for field and the doubles bit for bit, on the fixtures, on a seeded case of
20 000 sketches in clades of 50 and on a row long enough for the workgroup selection; a resident database; the capacity
convention; the error paths; consistency with finish_sparse()."""
import gzip, json, os, re, shutil, subprocess

import numpy as np
import pytest

import screen_results_model as model
from taxscreen_model import read_fastx
from mash_amd import abi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "screen_results")
IN = os.path.join(GOLD, "in")
MASH = os.path.join(ROOT, "mash_amd", "bin", "mash")
CASES = json.load(open(os.path.join(GOLD, "cases.json")))["screen"]

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch's HIP runtime initialises first when both live in one process -- before the model loads libmashgpu.so for
    the host p-value, which the command tests already do"""
    import torch
    torch.cuda.init()


@pytest.fixture(scope="module")
def eng(torch_first):
    e = abi.MashGpu(0)
    yield e
    e.close()


# ------------------------------------------------------------------------------------------------- the command
def _run(case, tmp_path, extra_env=None):
    env = dict(os.environ)
    env.pop("MASH_AMD_HOST_SCREEN_FINISH", None)
    env.pop("MASH_AMD_TIMING", None)
    env.update(extra_env or {})
    stdin = gzip.decompress(open(os.path.join(IN, case["stdin"]), "rb").read()) if case.get("stdin") else None
    r = subprocess.run([MASH, *case["cmd"]], cwd=tmp_path, capture_output=True, timeout=300, env=env, input=stdin)
    assert r.returncode == 0, (case["cmd"], r.stderr[-300:])
    return r


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_screen_cli_both_routes(case, tmp_path, oracle):
    assert os.path.exists(MASH), "mash_amd/bin/mash is not built"
    shutil.copytree(IN, tmp_path, dirs_exist_ok=True)
    for s in case["setup"]:
        r = subprocess.run([MASH, *s], cwd=tmp_path, capture_output=True, timeout=300)
        assert r.returncode == 0, (s, r.stderr[-300:])
    if case["parity"]:
        want = open(os.path.join(GOLD, case["name"] + ".out"), "rb").read()
    else:                              # a full tie: the reference's pick is its hash set's order, the model decides
        want = model.case_lines(oracle, case, IN)
    dev, host = _run(case, tmp_path), _run(case, tmp_path, {"MASH_AMD_HOST_SCREEN_FINISH": "1"})
    assert dev.stdout == want, case["name"]
    assert host.stdout == want, case["name"]
    assert dev.stderr == host.stderr
    for line in (b"Summing shared...", b"Computing coverage medians...", b"Writing output..."):
        assert line in dev.stderr
    assert (b"Reallocating to winners..." in dev.stderr) == ("-w" in case["cmd"])


def test_screen_cli_timing_laps_name_the_route(tmp_path):
    case = next(c for c in CASES if c["name"] == "winner")
    shutil.copytree(IN, tmp_path, dirs_exist_ok=True)
    for s in case["setup"]:
        assert subprocess.run([MASH, *s], cwd=tmp_path, capture_output=True, timeout=300).returncode == 0
    laps = lambda r: re.findall(r" ([a-z ]+?) [0-9.e+-]+ s;", [ln for ln in r.stderr.decode().splitlines() if ln.startswith("timing:") and ln.endswith(" s;")][-1])
    dev = laps(_run(case, tmp_path, {"MASH_AMD_TIMING": "1"}))
    host = laps(_run(case, tmp_path, {"MASH_AMD_TIMING": "1", "MASH_AMD_HOST_SCREEN_FINISH": "1"}))
    assert "results" in dev and "host tail" not in dev and dev[:2] == ["device", "screen"]
    assert "host tail" in host and "results" not in host and host[:2] == ["device", "screen"]


# ---------------------------------------------------------------------------------------------------- the C ABI
def _table(eng, rows, s, lengths):
    table = np.full((len(rows), s), np.uint64(abi.HASH_PAD), dtype=np.uint64)
    nhash = np.zeros(len(rows), dtype=np.uint32)
    for i, h in enumerate(rows):
        table[i, : len(h)] = h
        nhash[i] = len(h)
    return eng.table_upload(table, nhash, None if lengths is None else np.asarray(lengths, dtype=np.uint64))


def _bits(x):
    return int(np.array([x], dtype=np.float64).view(np.uint64)[0])


def _as_tuples(recs):
    return [(int(r["row"]), int(r["shared"]), int(r["denom"]), int(r["median"]), _bits(r["identity"]), _bits(r["p_value"])) for r in recs]


def _want(recs):
    return [(row, shared, denom, med, _bits(ident), _bits(pv)) for row, shared, denom, med, ident, pv in recs]


COMBOS = [(False, 0.0), (True, 0.0), (False, -1.0), (True, -1.0)]


def _check_all_combos(sc, hits, nhash, lengths, k, ssize, kspace, max_p=1.0):
    seen = []
    for winner, mi in COMBOS:
        want = _want(model.results(hits, nhash, lengths, k, ssize, kspace, winner=winner, min_identity=mi, max_p=max_p))
        recs, got_ss, _, _ = sc.results(kspace, winner=winner, min_identity=mi, max_p=max_p)
        assert got_ss == ssize
        got = _as_tuples(recs)
        assert len(got) == len(want), (winner, mi)
        for g, w in zip(got, want):
            assert g == w, (winner, mi, g, w)
        seen.append(got)
    return seen


@pytest.mark.parametrize("name", ["plain", "k11_plain", "clade_winner", "length_rule", "short_sketch", "protein", "full_tie", "two_files"])
def test_abi_equals_model_on_fixtures(eng, oracle, name):
    case = next(c for c in CASES if c["name"] == name)
    names, comments, lengths, rows, observed, mix = model.fixture_inputs(oracle, case, IN)
    aa = bool(case.get("protein"))
    kspace = float(20 if aa else 4) ** case["k"]
    p = eng.params(k=case["k"], s=case["s"], alphabet=model.PROTEIN if aa else "ACGT", noncanonical=aa)
    db = _table(eng, rows, case["s"], lengths)
    ssize = model.set_size(mix, 64 if kspace > 2.0 ** 32 else 32)
    hits = model.hits_of(rows, observed)
    with eng.screen_open(db, p, translate=aa) as sc:
        for pool in case["pools"]:
            sc.add_records([seq for _, _, seq in read_fastx(os.path.join(IN, pool))])
        seen = _check_all_combos(sc, hits, [len(r) for r in rows], lengths, case["k"], ssize, kspace)
        assert sum(t[1] for t in seen[0]) > 0
        _, _, got_mix, distinct = sc.results(kspace)
        assert np.array_equal(got_mix, np.array(mix, dtype=np.uint64)) and distinct == len({int(h) for r in rows for h in r})
        # the command's filters of this case, through the ABI
        winner, mi, mp = model.case_options(case)
        want = _want(model.results(hits, [len(r) for r in rows], lengths, case["k"], ssize, kspace, winner=winner, min_identity=mi, max_p=mp))
        assert _as_tuples(sc.results(kspace, winner=winner, min_identity=mi, max_p=mp)[0]) == want
    db.free()


def _hits_numpy(table, nhash, uniq, cnt):
    """[(row, count, hash)] of a table against the observed hashes (uniq ascending, cnt their multiplicities)"""
    n, s = table.shape
    valid = np.arange(s)[None, :] < nhash[:, None]
    at = np.minimum(np.searchsorted(uniq, table), len(uniq) - 1)
    hit = valid & (uniq[at] == table)
    r, c = np.nonzero(hit)
    return list(zip(r.tolist(), cnt[at[r, c]].tolist(), table[r, c].tolist()))


def _observed(oracle, reads, k):
    """(distinct k-mer hashes ascending, their multiplicities) of a list of reads, canonical nucleotide k-mers"""
    bases = np.frombuffer(b"".join(reads), dtype=np.uint8).copy()
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads], dtype=np.uint64)
    h = np.asarray(oracle.kmer_hashes(bases, off, oracle.params(k=k, s=1000)), dtype=np.uint64)
    return np.unique(h, return_counts=True)


def _clade_case(eng):
    """20 000 genomes of 1300 bases in clades of 50 (members at 0 - 5 % from their ancestor: holder runs of 1 .. 50), some rows
    cut to 600 bases (nhash < s), some rows copied under another length, some copied outright (full ties)"""
    rng = np.random.default_rng(20261018)
    n, per, L, s, k = 20_000, 50, 1300, 1000, 21
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    anc = acgt[rng.integers(0, 4, (n // per, L))]
    g = np.repeat(anc, per, axis=0)
    rate = np.tile(np.linspace(0.0, 0.05, per), n // per)
    mut = rng.random((n, L)) < rate[:, None]
    g[mut] = acgt[rng.integers(0, 4, int(mut.sum()))]
    length = np.full(n, L, dtype=np.uint64)
    length[rng.choice(n, 300, replace=False)] = 600
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(length)
    bases = np.concatenate([g[i, : int(length[i])] for i in range(n)])
    p = eng.params(k=k, s=s)
    table, nhash = eng.sketch_host_raw(bases, off, p)
    assert (nhash < s).sum() >= 300 and (nhash == s).sum() > n // 2
    lengths = length.copy()
    for j in rng.choice(n - 60, 200, replace=False):          # the same sketch a few rows on, under a larger / the same length
        table[j + 7], nhash[j + 7] = table[j], nhash[j]
        lengths[j + 7] = lengths[j] + (100 if j % 2 else 0)
    return g, table, nhash, lengths, p, s, k, rng


def test_abi_equals_model_on_clades(eng, oracle):
    g, table, nhash, lengths, p, s, k, rng = _clade_case(eng)
    n, L = g.shape
    src = np.concatenate([c * 50 + rng.choice(50, 20, replace=False) for c in rng.choice(n // 50, 100, replace=False)])   # a tenth of the genomes
    reads = []
    for i in src:
        for _ in range(1 + int(i) % 4):
            o = int(rng.integers(0, L - 300))
            reads.append(g[i, o : o + 300].tobytes())
    uniq, cnt = _observed(oracle, reads, k)
    hits = _hits_numpy(table, nhash, uniq, cnt)
    runs = np.unique(np.array([h for _, _, h in hits], dtype=np.uint64), return_counts=True)[1]
    assert runs.min() == 1 and runs.max() >= 40 and len(hits) > 500_000
    kspace = 4.0 ** k
    ssize = model.set_size(uniq[:s].tolist())
    db = eng.table_upload(table, nhash, lengths)
    with eng.screen_open(db, p) as sc:
        sc.add_records(reads)
        seen = _check_all_combos(sc, hits, nhash.tolist(), lengths.tolist(), k, ssize, kspace)
        assert len(seen[2]) == n and len(seen[0]) < n and seen[0] != seen[1]
        # filters after the reallocation
        want = _want(model.results(hits, nhash.tolist(), lengths.tolist(), k, ssize, kspace, winner=True, min_identity=0.8, max_p=1e-10))
        got = _as_tuples(sc.results(kspace, winner=True, min_identity=0.8, max_p=1e-10)[0])
        assert got == want and 0 < len(got) < len(seen[1])
    db.free()


def test_long_rows_take_every_branch_of_the_selection(eng, oracle):
    """s = 10 000, k = 31: a genome fully covered at uneven depth has 10 000 counts (a workgroup's selection, counts above
    255 so that two digits are looked at), its half-covered relative a few thousand, a short one a wave's"""
    rng = np.random.default_rng(7)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    s, k = 10_000, 31
    big = acgt[rng.integers(0, 4, 12_500)].tobytes()
    other = acgt[rng.integers(0, 4, 12_500)].tobytes()
    small = acgt[rng.integers(0, 4, 900)].tobytes()
    p = eng.params(k=k, s=s)
    table, nhash = eng.sketch_host([[big], [other], [small], [big[:6000] + other[6000:]]], p)
    assert nhash.tolist()[:2] == [s, s] and nhash[2] < s
    reads = [big] * 3 + [big[2000:9000]] * 300 + [big[4000:5000]] * 40 + [small] * 2 + [small[100:500]] * 5
    uniq, cnt = _observed(oracle, reads, k)
    assert cnt.max() > 256
    hits = _hits_numpy(table, nhash, uniq, cnt)
    lengths = [12_500, 12_500, 900, 12_500]
    db = eng.table_upload(table, nhash, np.array(lengths, dtype=np.uint64))
    with eng.screen_open(db, p) as sc:
        sc.add_records(reads)
        seen = _check_all_combos(sc, hits, nhash.tolist(), lengths, k, model.set_size(uniq[:s].tolist()), 4.0 ** k)
        shared = {t[0]: t[1] for t in seen[0]}
        assert shared[0] == s and 64 < shared[3] and 0 < shared[2] <= 900
        assert len({t[3] for t in seen[0]}) > 1
    db.free()


def test_resident_database_repeats_and_other_finishes(eng, oracle):
    case = next(c for c in CASES if c["name"] == "two_files")
    names, comments, lengths, rows, _, _ = model.fixture_inputs(oracle, case, IN)
    p = eng.params(k=case["k"], s=case["s"])
    db = _table(eng, rows, case["s"], lengths)
    kspace = 4.0 ** case["k"]
    mixtures = [[seq for _, _, seq in read_fastx(os.path.join(IN, f))] for f in ("pool_a.fa.gz", "pool_b.fq.gz")]
    fresh = []
    for mix in mixtures:
        with eng.screen_open(db, p) as sc:
            sc.add_records(mix)
            fresh.append([_as_tuples(sc.results(kspace, winner=w, min_identity=mi)[0]) for w, mi in COMBOS] + [sc.results(kspace)[1]])
    assert fresh[0][0] != fresh[1][0]
    with eng.screen_open(db, p) as sc:
        for mix, want in zip(mixtures, fresh):
            sc.add_records(mix)
            sparse_before = sc.finish_sparse()
            for (w, mi), exp in zip(COMBOS, want):
                assert _as_tuples(sc.results(kspace, winner=w, min_identity=mi)[0]) == exp
            assert _as_tuples(sc.results(kspace)[0]) == want[0] and sc.results(kspace)[1] == want[4]      # asking again changes nothing
            some = _as_tuples(sc.results(kspace, min_identity=0.99)[0])
            assert some == [t for t in want[0] if np.array([t[4]], dtype=np.uint64).view(np.float64)[0] >= 0.99] and len(some) < len(want[0])
            sparse_after = sc.finish_sparse()
            assert np.array_equal(sparse_before[0], sparse_after[0]) and np.array_equal(sparse_before[1], sparse_after[1])
            sc.reset()
        empty, ssize, mix, _ = sc.results(kspace, min_identity=-1.0)
        assert ssize == 0 and len(mix) == 0 and len(empty) == len(rows)
        assert all(int(r["shared"]) == 0 and r["identity"] == 0.0 and r["p_value"] == 1.0 and int(r["median"]) == 0 for r in empty)
        assert [int(r["row"]) for r in empty] == list(range(len(rows))) and [int(r["denom"]) for r in empty] == [len(r) for r in rows]
        assert len(sc.results(kspace)[0]) == 0
    # beside the taxon counts of the same screen
    t = eng.taxonomy(np.zeros(3, dtype=np.uint32))
    with eng.screen_open(db, p) as sc:
        sc.set_taxa(t, np.array([1 + i % 2 for i in range(len(rows))], dtype=np.uint32))
        sc.add_records(mixtures[0])
        tax_before = sc.tax_finish()
        assert _as_tuples(sc.results(kspace, winner=True)[0]) == fresh[0][1]
        tax_after = sc.tax_finish()
        assert [tuple(x) for x in tax_before[0].tolist()] == [tuple(x) for x in tax_after[0].tolist()] and tax_before[1:3] == tax_after[1:3]
        assert _as_tuples(sc.results(kspace)[0]) == fresh[0][0]
    t.free()
    db.free()


def _code(excinfo):
    return int(re.search(r"error (-?\d+)", str(excinfo.value)).group(1))


def test_capacity_convention_and_errors(eng, oracle):
    case = next(c for c in CASES if c["name"] == "plain")
    names, comments, lengths, rows, _, _ = model.fixture_inputs(oracle, case, IN)
    p = eng.params(k=case["k"], s=case["s"])
    kspace = 4.0 ** case["k"]
    reads = [seq for _, _, seq in read_fastx(os.path.join(IN, "pool_a.fa.gz"))]
    db = _table(eng, rows, case["s"], lengths)
    with eng.screen_open(db, p) as sc:
        sc.add_records(reads)
        full = _as_tuples(sc.results(kspace, winner=True)[0])
        assert len(full) >= 3
        sized = sc.results(kspace, winner=True, capacity=0)
        assert len(sized[0]) == 0 and sized[4] == len(full)
        short = sc.results(kspace, winner=True, capacity=2)
        assert _as_tuples(short[0]) == full[:2] and short[4] == len(full)
        exact = sc.results(kspace, winner=True, capacity=len(full))
        assert _as_tuples(exact[0]) == full and exact[4] == len(full)
        roomy = sc.results(kspace, winner=True, capacity=len(full) + 50)
        assert _as_tuples(roomy[0]) == full
    db.free()
    bare = _table(eng, rows, case["s"], None)                                      # uploaded without lengths
    with eng.screen_open(bare, p) as sc:
        sc.add_records(reads)
        with pytest.raises(abi.MashGpuError) as e:
            sc.results(kspace, winner=True)
        assert _code(e) == -1 and "lengths" in str(e.value)
        plain = _as_tuples(sc.results(kspace)[0])                                  # and the same screen still answers without -w
        assert [t[:4] for t in plain] == [t[:4] for t in _as_tuples(sc.results(kspace, capacity=len(plain))[0])] and len(plain) >= 3
    bare.free()


def test_consistent_with_the_sparse_finish(eng, oracle):
    case = next(c for c in CASES if c["name"] == "clade_winner")
    names, comments, lengths, rows, _, _ = model.fixture_inputs(oracle, case, IN)
    p = eng.params(k=case["k"], s=case["s"])
    db = _table(eng, rows, case["s"], lengths)
    with eng.screen_open(db, p) as sc:
        sc.add_records([seq for _, _, seq in read_fastx(os.path.join(IN, "pool_clade.fa.gz"))])
        recs = sc.results(4.0 ** case["k"], min_identity=-1.0)[0]
        hits = sc.finish_sparse()[0]
        assert len(recs) == len(rows)
        for r in recs:
            mine = np.sort(hits["count"][hits["row"] == r["row"]])
            assert int(r["shared"]) == len(mine)
            assert int(r["median"]) == (int(mine[len(mine) // 2]) if len(mine) else 0)
    db.free()
