"""`mash taxscreen` / `mash bounds` on the GPU, judged by tests/taxscreen_model.py and by the recorded stdout of the
reference CLI (tests/golden/taxscreen; tests/test_taxscreen_model.py shows on the CPU that the two agree on every parity
fixture).  Through the command: every parity fixture byte for byte, the model's bytes for the `defect` fixture.  Through
the C ABI: the per-hash LCA nodes and the per-taxon counts equal the model on the fixtures and on a seeded random case
that takes the long-run path; a resident database; the capacity convention; the error paths."""
import json, os, re, shutil, subprocess

import numpy as np
import pytest

import taxscreen_model as model
from mash_amd import abi
from workloads import synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "taxscreen")
IN = os.path.join(GOLD, "in")
MASH = os.path.join(ROOT, "mash_amd", "bin", "mash")
ALL = json.load(open(os.path.join(GOLD, "cases.json")))
CASES, BOUNDS = ALL["taxscreen"], ALL["bounds"]

# cases where this CLI is known to print something else than the reference (none may be added silently: each entry
# says what differs)
KNOWN_DIFFERENCES = {}

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch                       # (torch's HIP runtime initialises first when both live in one process)
    torch.cuda.init()
    e = abi.MashGpu(0)
    yield e
    e.close()


def _model_inputs(oracle, case):
    names, comments, rows, observed = model.fixture_sets(oracle, case, IN)
    tax = model.parse_taxonomy(os.path.join(IN, case["taxdir"], "nodes.dmp"), os.path.join(IN, case["taxdir"], "names.dmp"))
    ids = model.reference_taxids(names, comments, os.path.join(IN, case["mapping"]) if case["mapping"] else None)
    return tax, ids, rows, observed


# ------------------------------------------------------------------------------------------------- the commands
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_taxscreen_cli(case, tmp_path, oracle):
    if case["name"] in KNOWN_DIFFERENCES:
        pytest.xfail(KNOWN_DIFFERENCES[case["name"]])
    assert os.path.exists(MASH), "mash_amd/bin/mash is not built"
    shutil.copytree(IN, tmp_path, dirs_exist_ok=True)
    for s in case["setup"]:
        r = subprocess.run([MASH, *s], cwd=tmp_path, capture_output=True, timeout=300)
        assert r.returncode == 0, (s, r.stderr[-300:])
    r = subprocess.run([MASH, *case["cmd"]], cwd=tmp_path, capture_output=True, timeout=300)
    assert r.returncode == 0, (case["cmd"], r.stderr[-300:])
    if case["parity"]:
        want = open(os.path.join(GOLD, case["name"] + ".out"), "rb").read()
    else:                              # the reference counts clades twice here (see test_taxscreen_model.py): the model decides
        want = model.report(*_model_inputs(oracle, case))
    assert r.stdout == want, case["name"]


def test_taxscreen_cli_stdin_and_exit_statuses(tmp_path):
    case = next(c for c in CASES if c["name"] == "comment_taxids")
    shutil.copytree(IN, tmp_path, dirs_exist_ok=True)
    for s in case["setup"]:
        assert subprocess.run([MASH, *s], cwd=tmp_path, capture_output=True, timeout=300).returncode == 0
    want = open(os.path.join(GOLD, case["name"] + ".out"), "rb").read()
    pool = open(os.path.join(IN, "pool_a.fa"), "rb").read()
    r = subprocess.run([MASH, "taxscreen", "-t", "tax_bal", "bal.msh", "-"], cwd=tmp_path, input=pool, capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stdout == want
    r = subprocess.run([MASH, "taxscreen", "-t", "tax_bal", "bal.msh", "pool_a.fa", "-"], cwd=tmp_path, input=pool, capture_output=True, timeout=300)
    assert r.returncode == 1 and b"must be first" in r.stderr
    r = subprocess.run([MASH, "taxscreen", "-t", "nowhere", "bal.msh", "pool_a.fa"], cwd=tmp_path, capture_output=True, timeout=300)
    assert r.returncode == 1 and b"names.dmp or nodes.dmp" in r.stderr and r.stdout == b""
    r = subprocess.run([MASH, "taxscreen", "-t", "tax_bal", "bal.fa.gz", "pool_a.fa"], cwd=tmp_path, capture_output=True, timeout=300)
    assert r.returncode == 1 and b"does not look like a sketch" in r.stderr
    r = subprocess.run([MASH, "taxscreen", "bal.msh"], cwd=tmp_path, capture_output=True, timeout=300)
    assert r.returncode == 0 and b"mash taxscreen" in r.stdout


@pytest.mark.parametrize("case", BOUNDS, ids=[c["name"] for c in BOUNDS])
def test_bounds_cli(case):
    if case["name"] in KNOWN_DIFFERENCES:
        pytest.xfail(KNOWN_DIFFERENCES[case["name"]])
    r = subprocess.run([MASH, *case["cmd"]], capture_output=True, timeout=300)
    assert r.returncode == 0
    assert r.stdout == open(os.path.join(GOLD, case["name"] + ".out"), "rb").read()


# ---------------------------------------------------------------------------------------------------- the C ABI
def _dense_taxonomy(tax, ids):
    """taxIDs -> dense nodes (ascending taxID); rows whose taxID the taxonomy lacks get TAX_NONE"""
    order = sorted(tax)
    idx = {t: i for i, t in enumerate(order)}
    parent = np.array([idx[t] if tax[t][0] is None else idx[tax[t][0]] for t in order], dtype=np.uint32)
    row_node = np.array([idx.get(t, abi.TAX_NONE) for t in ids], dtype=np.uint32)
    return parent, row_node


def _table(eng, rows, s):
    table = np.full((len(rows), s), np.uint64(abi.HASH_PAD), dtype=np.uint64)
    nhash = np.zeros(len(rows), dtype=np.uint32)
    for i, h in enumerate(rows):
        table[i, : len(h)] = h
        nhash[i] = len(h)
    return eng.table_upload(table, nhash, np.full(len(rows), 1000, dtype=np.uint64))


def _as_tuples(taxa):
    return [tuple(int(x) for x in t) for t in taxa]


def _check_against_model(sc, parent, rows, row_node, observed):
    hn = model.hash_nodes(list(parent), rows, row_node)
    hashes, nodes = sc.hash_taxa()
    assert np.array_equal(hashes, np.array(sorted(hn), dtype=np.uint64))
    assert np.array_equal(nodes, np.array([hn[h] for h in sorted(hn)], dtype=np.uint32))
    want, total, total_hash = model.taxon_counts(list(parent), hn, observed)
    taxa, got_total, got_total_hash, _, distinct = sc.tax_finish()
    assert _as_tuples(taxa) == want
    assert (got_total, got_total_hash, distinct) == (total, total_hash, len(hn))
    return want


@pytest.mark.parametrize("name", ["balanced", "no_taxid", "defect", "protein_six_frames"])
def test_abi_equals_model_on_fixtures(eng, oracle, name):
    case = next(c for c in CASES if c["name"] == name)
    tax, ids, rows, observed = _model_inputs(oracle, case)
    parent, row_node = _dense_taxonomy(tax, ids)
    aa = bool(case.get("protein"))
    p = eng.params(k=case["k"], s=case["s"], alphabet=model.PROTEIN if aa else "ACGT", noncanonical=aa)
    db = _table(eng, rows, case["s"])
    t = eng.taxonomy(parent)
    with eng.screen_open(db, p, translate=aa) as sc:
        sc.set_taxa(t, row_node)
        for pool in case["pools"]:
            sc.add_records([seq for _, _, seq in model.read_fastx(os.path.join(IN, pool))])
        want = _check_against_model(sc, parent, rows, row_node, observed)
        assert sum(w[1] for w in want) > 0
    t.free()
    db.free()


def _random_case(oracle):
    rng = np.random.default_rng(20261016)
    n_nodes, n, s = 100_000, 3000, 200
    parent = np.zeros(n_nodes, dtype=np.uint32)
    parent[1] = 1                                                  # a second root
    parent[2:64] = np.arange(1, 63)                                # a chain under it: depth past 60
    lo = np.maximum(0, np.arange(64, n_nodes) - 2000)
    parent[64:] = (lo + rng.integers(0, 2000, n_nodes - 64) % (np.arange(64, n_nodes) - lo)).astype(np.uint32)
    depth = model.depths(list(parent))
    assert max(depth) > 30 and sum(1 for i in range(n_nodes) if parent[i] == i) == 2
    table, nhash, _ = synth.clustered_sketches(n, s, clusters=30, seed=5, pool=260, private=80)
    rows = [table[i, : nhash[i]] for i in range(n)]
    # real k-mer hashes planted into the rows, so that a mixture can observe them
    seq = synth._rand_dna(rng, 20000)
    op = oracle.params(k=21, s=100000)
    real = oracle.sketch_records([seq], op)[0]
    seen = oracle.sketch_records([seq[:9000]], op)[0]
    shared = seen[0]                                               # one hash held by 1500 rows: the long-run path
    holders = set(rng.choice(n, 1500, replace=False).tolist())
    for i in range(n):
        plant = real[rng.integers(0, len(real), 30)]
        if i in holders:
            plant = np.append(plant, shared)
        rows[i] = np.unique(np.concatenate([rows[i][: s - 40], plant]))[:s]
        if i in holders and shared not in rows[i]:
            rows[i][-1] = shared
            rows[i] = np.unique(rows[i])
    row_node = rng.integers(0, n_nodes, n).astype(np.uint32)
    row_node[rng.random(n) < 0.05] = abi.TAX_NONE
    row_node[::50] = rng.integers(2, 64, len(row_node[::50]))      # some rows on the deep chain
    return parent, rows, row_node, seq, set(int(x) for x in seen), s


def test_abi_equals_model_on_a_random_forest(eng, oracle):
    parent, rows, row_node, seq, observed, s = _random_case(oracle)
    p = eng.params(k=21, s=s)
    db = _table(eng, rows, s)
    t = eng.taxonomy(parent)
    with eng.screen_open(db, p) as sc:
        sc.set_taxa(t, row_node)
        m = re.search(r"(\d+) long runs", sc.tax_note())
        assert m and int(m.group(1)) >= 1, sc.tax_note()
        sc.add_records([seq[:9000]])
        want = _check_against_model(sc, parent, rows, row_node, observed)
        assert sum(w[1] for w in want) > 100
        assert any(w[0] == abi.TAX_DISJOINT for w in want) and any(w[0] == abi.TAX_NONE for w in want)
    t.free()
    db.free()


def test_resident_database_and_capacity(eng, oracle):
    case = next(c for c in CASES if c["name"] == "three_pools")
    tax, ids, rows, _ = _model_inputs(oracle, case)
    parent, row_node = _dense_taxonomy(tax, ids)
    p = eng.params(k=case["k"], s=case["s"])
    db = _table(eng, rows, case["s"])
    t = eng.taxonomy(parent)
    mixtures = [[seq for _, _, seq in model.read_fastx(os.path.join(IN, f))] for f in ("pool_a.fa", "pool_c.fa.gz")]
    fresh = []
    for mix in mixtures:
        with eng.screen_open(db, p) as sc:
            sc.set_taxa(t, row_node)
            sc.add_records(mix)
            fresh.append(sc.tax_finish())
    assert _as_tuples(fresh[0][0]) != _as_tuples(fresh[1][0])
    with eng.screen_open(db, p) as sc:
        sc.set_taxa(t, row_node)
        note = sc.tax_note()
        assert "built 1 time" in note
        for mix, want in zip(mixtures, fresh):
            sc.add_records(mix)
            got = sc.tax_finish()
            assert _as_tuples(got[0]) == _as_tuples(want[0]) and got[1:3] == want[1:3] and np.array_equal(got[3], want[3])
            assert _as_tuples(sc.tax_finish()[0]) == _as_tuples(want[0])          # asking twice changes nothing
            sc.reset()
        assert sc.tax_note() == note                                            # the per-hash LCA was not recomputed
        empty = sc.tax_finish()
        assert empty[1] == 0 and all(x[1] == 0 and x[3] == 0 for x in _as_tuples(empty[0])) and empty[2] == fresh[0][2]
        # capacity: sizing call, short buffer, exact buffer
        sc.add_records(mixtures[0])
        full = _as_tuples(fresh[0][0])
        sized = sc.tax_finish(capacity=0)
        assert len(sized[0]) == 0 and sized[5] == len(full) and sized[1] == fresh[0][1]
        short = sc.tax_finish(capacity=3)
        assert _as_tuples(short[0]) == full[:3] and short[5] == len(full)
        exact = sc.tax_finish(capacity=len(full))
        assert _as_tuples(exact[0]) == full and exact[5] == len(full)
    t.free()
    db.free()


def _code(excinfo):
    return int(re.search(r"error (-?\d+)", str(excinfo.value)).group(1))


def test_error_paths_leave_the_context_usable(eng, oracle):
    with pytest.raises(abi.MashGpuError) as e:
        eng.taxonomy(np.array([0, 2, 3, 1], dtype=np.uint32))                   # 1 -> 2 -> 3 -> 1
    assert _code(e) == -1 and "cycle" in str(e.value)
    with pytest.raises(abi.MashGpuError) as e:
        eng.taxonomy(np.array([0, 0, 7], dtype=np.uint32))
    assert _code(e) == -1 and "out of range" in str(e.value)
    rows = [np.array([5, 6, 7], dtype=np.uint64), np.array([6, 9], dtype=np.uint64)]
    db = _table(eng, rows, 4)
    p = eng.params(k=21, s=4)
    t = eng.taxonomy(np.array([0, 0, 0], dtype=np.uint32))
    with eng.screen_open(db, p) as sc:
        with pytest.raises(abi.MashGpuError) as e:
            sc.tax_finish()
        assert _code(e) == -1 and "set_taxa" in str(e.value)
        with pytest.raises(abi.MashGpuError) as e:
            sc.hash_taxa()
        assert _code(e) == -1
        with pytest.raises(abi.MashGpuError) as e:
            sc.set_taxa(t, np.array([1, 2, 1], dtype=np.uint32))                # three nodes for two rows
        assert _code(e) == -1 and "rows" in str(e.value)
        with pytest.raises(abi.MashGpuError) as e:
            sc.set_taxa(t, np.array([1, 3], dtype=np.uint32))
        assert _code(e) == -1 and "out of range" in str(e.value)
        sc.set_taxa(t, np.array([1, 2], dtype=np.uint32))                       # and the same objects still work
        hashes, nodes = sc.hash_taxa()
        assert hashes.tolist() == [5, 6, 7, 9] and nodes.tolist() == [1, 0, 1, 2]
        taxa, total, total_hash, _, distinct = sc.tax_finish()
        assert _as_tuples(taxa) == [(0, 0, 1, 0, 4), (1, 0, 2, 0, 2), (2, 0, 1, 0, 1)] and (total, total_hash, distinct) == (0, 4, 4)
    t.free()
    db.free()
