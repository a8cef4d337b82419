"""Every merge form of the inverted-index engine (compare_sparse.hip) on the device, through the C ABI, against the oracle.

SparseJobRun::merge_and_scatter picks one of six kernels by the table's shape and by knobs no other test sets: one lane per
candidate (`lanes`, reachable through MASHGPU_SPARSE_MERGE only), the whole row in LDS (`rows`), the row a window of 2048 codes
at a time (`rows windowed`: row strides above 2056, or MASHGPU_SPARSE_MERGE_WINDOWS), several rows per work item (`pack 32 | 43 |
64`: MASHGPU_SPARSE_PACK_MIN).  Here every form runs on tables built for the kernels' edges -- the recipes of
tests/emu/sparse_emu_main.cpp, which runs the same kernels on the CPU --, with dense groups and the join engine off so that
every pair that shares a hash goes through the merge.  Every pair is compared with the oracle (integers: no tolerance); the
MASHGPU_SPARSE_DBG line of merge_and_scatter must name the form that was asked for (or, where the launcher has to decline --
pack and rows at s >= 2053 --, the one that took over) and the candidate count the table gives; the six forms' outputs of one
table have the same bytes."""
import re

import numpy as np
import pytest

from mash_amd import abi
from tests import helpers
from tests.helpers import _check_records_against_oracle, _oracle_pass, _same_bits, tri_base

pytestmark = pytest.mark.gpu

K, KSPACE21 = 21, 4.0 ** 21
PAD = 0xFFFFFFFFFFFFFFFF

# form -> (context options, process-wide knobs read at every launch)
FORMS = {"lanes": ({"MASHGPU_SPARSE_MERGE": "lanes"}, {}),
         "rows": ({"MASHGPU_SPARSE_MERGE_PACK": "0"}, {}),
         "rows windowed": ({"MASHGPU_SPARSE_MERGE_PACK": "0"}, {"MASHGPU_SPARSE_MERGE_WINDOWS": "1"}),
         "pack 32": ({"MASHGPU_SPARSE_MERGE_PACK": "1"}, {"MASHGPU_SPARSE_PACK_MIN": "32"}),
         "pack 43": ({"MASHGPU_SPARSE_MERGE_PACK": "1"}, {"MASHGPU_SPARSE_PACK_MIN": "43"}),
         "pack 64": ({"MASHGPU_SPARSE_MERGE_PACK": "1"}, {"MASHGPU_SPARSE_PACK_MIN": "64"})}
TABLES = ["sizes", "ring", "chunks", "pack", "windows", "copies"]
WHOLE_ROW_MOST = 2052                  # s = 2052 gives a row stride of 2056, the largest the whole-row and pack kernels stage


# ------------------------------------------------------------------------------------------ the tables (sparse_emu_main.cpp's recipes)

def V(k):
    """value number k: ascending in k, above 2^32, low bits that do not follow k"""
    return ((k + 1) << 34) + ((k * 2654435761) & 0xFFFFFFFF)


def span(first, count, stride=1):
    return [V(first + k * stride) for k in range(count)]


def finish(v, keep):
    return sorted(set(v))[:keep]


def table_sizes(s):
    """rows of every length 0 .. s over one pool of 2 s + 3 values; row 0 is full, the last row is not empty"""
    n, P = max(40, s + 2), 2 * s + 3
    t = []
    for r in range(n):
        L = s - r % (s + 1)
        if r == n - 1 and L == 0:
            L = s
        start, step = (3 * r) % P, 1 + (r & 1)
        t.append([V(1000 + (start + k * step) % P) for k in range(L)])
    return t


def table_ring():
    """s = 200: what the ring of 32 codes and its refill of eight a round can meet"""
    M = span(20000, 200)
    t = [span(0, 199) + [M[0]],                 # a column below the row: ib advances 8 every round
         [M[0]] + span(40000, 199),             # a column above the row: its ring stalls full
         M]
    for run in (9, 17, 33):                     # runs of 9, 17, 33 values alternate between the two sides
        b = 50000 + 1000 * run
        x, y, k = [V(b)], [V(b)], 0
        while len(x) < 200 or len(y) < 200:
            side = y if (k // run) % 2 else x
            if len(side) < 200:
                side.append(V(b + 1 + k))
            k += 1
        t += [x, y]
    t += [span(60000, 200), span(60000, 200)]   # the same row twice
    b = 61000                                   # a side exhausted at union size 17, 23, 24, 25, as column and as row
    for role in (0, 1):
        for u in (17, 23, 24, 25):
            if u % 2 == 0:
                m = u // 2
                lng, sht = [V(b)] + span(b + 2, 199, 2), [V(b)] + span(b + 1, m - 1, 2) + [V(b + 2 * m - 1)]
            else:
                m = (u - 1) // 2
                lng, sht = span(b + 2, 200, 2), span(b + 1, m, 2) + [V(b + 2 * m + 2)]
            t += [sht, lng] if role == 0 else [lng, sht]
            b += 1000
    for c in range(64):                         # 63 columns 200 codes from any bound, one with five codes in all
        t.append([V(70000), V(70002), V(70005), V(70006), V(70008)] if c == 40 else [V(70000 + 2 * k + ((k + c) % 2)) for k in range(200)])
    t.append(span(70000, 200, 2))
    return t


def table_chunks():
    """s = 8: rows with 1 .. 256 candidates (leaf k shares a tag with every leaf below it) and with exactly 127, 128, 129, 256, 257"""
    ms = (127, 128, 129, 256, 257)

    def G(i):
        return V(10 + i) if i < 2 else V(900000 + i)
    t = [span(1000 + 10 * k, 3) + [G(i) for i in range(5) if ms[i] > k] for k in range(257)]
    return t + [[G(i)] + span(500000 + 10 * i, 7) for i in range(5)]


PACK_COUNTS = (0, 1, 31, 32, 33, 0, 0, 42, 43, 44, 63, 64, 65, 127, 128, 129, 300, 1, 1, 1, 1, 1, 1, 1, 1)


def table_pack():
    """s = 300: 300 leaves that share nothing with each other, then rows with exactly PACK_COUNTS[i] candidates among the leaves,
    the first of the list last in the table (visited first without an order)"""
    t = [span(1000 + 32 * k, 25) for k in range(300)]
    for i in range(24, -1, -1):
        t.append(span(100000 + 8 * i, 2) + [V(1000 + 32 * k + i) for k in range(PACK_COUNTS[i])])
    return t


def table_windows(s):
    """rows of 2047, 2048, 2049, 4096, 4097 values (at most s) and short ones over one pool; in front of them four columns made for
    the last row A: denom reaches s exactly at ia = 2048, a column exhausted exactly at the window's edge, a lane done in the first
    window and one that needs the last"""
    Ls = (2047, 2048, 2049, 4096, 4097, 5, 100, 0)
    body = []
    for r in range(16):
        L, v, k = min(4097 if r == 15 else Ls[r % 8], s), [], 0
        while len(v) < L:
            if (k + r) % 4 != 0:
                v.append(V(5000 + k))
            k += 1
        body.append(v)
    A, t = body[-1], []
    if len(A) >= 2048:
        t += [span(0, s - 2048) + [A[2047]], A[2040:2048]]
    return t + [[A[0]], [A[-1]]] + body


def table_copies():
    """s = 40, 110 rows over one pool: classes of 2, 3 and 70 rows, one of them of a short row"""
    t = []
    for r in range(110):
        L, start, step = 40 - r % 7, (5 * r) % 83, 1 + (r & 1)
        t.append(finish([V(1000 + (start + k * step) % 83) for k in range(L)], 40))
    t[5] = t[5][:3]
    t[107] = t[5]
    t[50] = t[10]
    t[30] = t[99] = t[11]
    for r in range(35, 104):
        if r not in (50, 99):
            t[r] = t[34]
    t[104] = t[105] = t[34]
    return t


def tables_rect():
    """s = 32: 45 reference rows (a value of its own in front of each and another between the pool's values, then values of an
    even-numbered pool), copies among them; queries below every table value, above, between two, equal to a value of one row and
    of many, empty, and rows of the table itself"""
    ref = []
    for r in range(45):
        L, start, step = 31 - r % 5, (7 * r) % 71, 1 + (r & 1)
        ref.append(finish([V(900 + r), V(1001 + 2 * r)] + [V(1000 + 2 * ((start + k * step) % 71)) for k in range(L)], 32))
    ref[40] = ref[41] = ref[3]
    ref[7] = ref[44]
    qry = [span(0, 32), span(0, 31) + [V(900 + 12)], [V(1000 + 2 * 20)] + span(5000, 31), span(1091, 26, 2), span(1000, 32), [],
           [V(900 + 3)] + span(6000, 3), [V(1000 + 2 * 70)]]
    qry += [ref[r] for r in (0, 3, 7, 20, 44)]
    for r in range(0, 45, 4):
        qry.append(ref[r][: len(ref[r]) // 2 + r % 3] + span(1001 + 2 * r, 6, 2))
    return ref, [finish(v, 32) for v in qry]


def _arrays(rows, s, width=None):
    rows = [finish(r, s) for r in rows]
    table = np.full((len(rows), width or s), PAD, dtype=np.uint64)
    nhash = np.zeros(len(rows), dtype=np.uint32)
    for i, r in enumerate(rows):
        table[i, : len(r)] = np.array(r, dtype=np.uint64)
        nhash[i] = len(r)
    return rows, table, nhash


def _shares(rows, copies_too=False):
    """bool [n, n], lower triangle: the two rows have a value in common and are not copies of each other (copies_too: or are)"""
    n = len(rows)
    M = np.zeros((n, n), dtype=bool)
    holders, classes = {}, {}
    for i, r in enumerate(rows):
        for v in r:
            holders.setdefault(v, []).append(i)
        if r:
            classes.setdefault(tuple(r), []).append(i)
    for h in holders.values():
        if len(h) > 1:
            M[np.ix_(h, h)] = True
    if not copies_too:
        for g in classes.values():
            M[np.ix_(g, g)] = False
    return np.tril(M, -1)


def _tri_case(oracle, rows, s, rng):
    rows, table, nhash = _arrays(rows, s)
    n = len(rows)
    lengths = rng.integers(10 ** 4, 10 ** 8, n).astype(np.uint64)
    c = {"rows": rows, "table": table, "nhash": nhash, "lengths": lengths, "n": n, "s": s, "shares": _shares(rows)}
    c["numer"], c["denom"], c["dist"], c["pval"] = oracle.triangle(table, nhash, lengths, 0, n, K, KSPACE21, stats=True)
    c["counts"] = np.zeros(len(c["numer"]), dtype=abi.COUNTS_DTYPE)
    c["counts"]["numer"], c["counts"]["denom"] = c["numer"], c["denom"]
    c["range"] = (n // 3, n - n // 5)                       # a proper range: neither row 0 nor the last row
    if not c["shares"][c["range"][0]:c["range"][1]].any():  # (pack: the rows with candidates are the table's last 25)
        c["range"] = (n // 2, n - 5)
    return c


SIZES_S = (1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 24, 25, 31, 32, 33, 40, 63, 64, 65)
WINDOWS_S = (2044, 2048, 2052, 2053, 4096, 4100)


@pytest.fixture(scope="module")
def cases(oracle):
    """table name -> its cases (one per sketch size) with the oracle's whole triangle; made once, on first use, read-only"""
    memo = {}
    make = {"sizes": lambda: [(table_sizes(s), s) for s in SIZES_S], "ring": lambda: [(table_ring(), 200)], "chunks": lambda: [(table_chunks(), 8)],
            "pack": lambda: [(table_pack(), 300)], "windows": lambda: [(table_windows(s), s) for s in WINDOWS_S], "copies": lambda: [(table_copies(), 40)]}

    def get(name):
        if name not in memo:
            rng = np.random.default_rng(5)
            memo[name] = [_tri_case(oracle, rows, s, rng) for rows, s in make[name]()]
            for c in memo[name]:
                for v in c.values():
                    if isinstance(v, np.ndarray):
                        v.flags.writeable = False
        return memo[name]
    return get


@pytest.fixture(scope="module")
def eng():
    import torch
    torch.cuda.init()          # (torch ships its own HIP runtime: it initialises first, tests/test_gpu_parity.py)
    e = abi.MashGpu(0)
    e.set_option("MASHGPU_COSTS_FIXED", "1")
    yield e
    e.close()


@pytest.fixture
def merge_form(eng, monkeypatch):
    """sets a merge form (and: the index engine, no dense groups, no join engine, the debug lines) for one test"""
    def use(form):
        monkeypatch.setenv("MASHGPU_COMPARE_KERNEL", "sparse")
        monkeypatch.setenv("MASHGPU_COMPARE_DENSE", "0")     # host_index.cpp: atoi(v) != 0 turns the groups on
        monkeypatch.setenv("MASHGPU_COMPARE_JOIN", "0")      # host_compare.cpp: atoi(e) == 0 keeps the join engine out
        monkeypatch.setenv("MASHGPU_SPARSE_DBG", "1")
        for v in ("MASHGPU_SPARSE_MERGE_WINDOWS", "MASHGPU_SPARSE_PACK_MIN", "MASHGPU_SPARSE_MERGE", "MASHGPU_SPARSE_MERGE_PACK"):
            monkeypatch.delenv(v, raising=False)
        opts, env = FORMS[form]
        for k, v in opts.items():
            eng.set_option(k, v)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    yield use
    for k in ("MASHGPU_SPARSE_MERGE", "MASHGPU_SPARSE_MERGE_PACK"):
        eng.set_option(k, None)


def _merge_lines(err):
    """[(form, candidates, for lists)] of the merge_and_scatter debug lines"""
    return [(m[0], int(m[1]), bool(m[2])) for m in re.findall(r"^compare merge: (.+?), (\d+) candidates( \(for lists\))?$", err, re.M)]


def _takes_over(form, s):
    return "rows windowed" if form != "lanes" and s > WHOLE_ROW_MOST else form


_outputs = {}                                               # (table, case, range) -> the first form's bytes


def _same_as_the_other_forms(key, got):
    first = _outputs.setdefault(key, got.copy())
    assert _same_bits(first, got), key


def _check_tri(got, c, rb, re, what):
    want = c["counts"][tri_base(rb):tri_base(re)]
    if got.tobytes() != want.tobytes():
        bad = np.nonzero((got["numer"] != want["numer"]) | (got["denom"] != want["denom"]))[0]
        rows, cols = helpers.tri_rows_cols(rb, re)
        first = [(int(rows[i]), int(cols[i]), tuple(got[i]), tuple(want[i])) for i in bad[:5]]
        raise AssertionError(f"{what} rows [{rb}, {re}): {len(bad)} of {len(want)} pairs differ from the oracle; (row, col, got, want): {first}")


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("table", TABLES)
def test_merge_form_on_a_table_made_for_its_edges(eng, cases, merge_form, capfd, monkeypatch, table, form):
    merge_form(form)
    for k, c in enumerate(cases(table)):
        n, s = c["n"], c["s"]
        tab = eng.table_upload(c["table"], c["nhash"], c["lengths"])
        try:
            for rb, re in ((0, n), c["range"]):
                capfd.readouterr()
                got = eng.compare_tri_host(tab, rb, re)
                lines = _merge_lines(capfd.readouterr().err)
                what = (table, s, form)
                _check_tri(got, c, rb, re, what)
                cand = int(c["shares"][rb:re].sum())
                assert cand > 0 or s == 1, (what, rb, re)
                assert lines == ([(_takes_over(form, s), cand, False)] if cand else []), (what, rb, re, lines)
                _same_as_the_other_forms((table, k, rb, re), got)
            if s == 1:
                # two rows of one value that share it are copies of each other: no candidate above.  Without classes
                # (MASHGPU_SPARSE_NO_DEDUP) they are merged like any pair.
                monkeypatch.setenv("MASHGPU_SPARSE_NO_DEDUP", "1")
                tab.invalidate()
                capfd.readouterr()
                got = eng.compare_tri_host(tab, 0, n)
                lines = _merge_lines(capfd.readouterr().err)
                monkeypatch.delenv("MASHGPU_SPARSE_NO_DEDUP")
                _check_tri(got, c, 0, n, (table, s, form, "no classes"))
                cand = int(_shares(c["rows"], copies_too=True).sum())
                assert cand > 0 and lines == [(form, cand, False)], (table, s, form, lines)
        finally:
            tab.free()


@pytest.fixture(scope="module")
def rect_cases(oracle):
    """the rect tables at query sketch sizes 32, 20 and 48 (the compare runs at the smaller of the two tables' sizes)"""
    ref, qry = tables_rect()
    rng = np.random.default_rng(6)
    _, rt, rn = _arrays(ref, 32)
    rl = rng.integers(10 ** 4, 10 ** 8, len(ref)).astype(np.uint64)
    ql = rng.integers(10 ** 4, 10 ** 8, len(qry)).astype(np.uint64)
    out = []
    for sq in (32, 20, 48):
        _, qt, qn = _arrays(qry, min(sq, 32), width=sq)
        s = min(32, sq)
        numer, denom, _, _ = helpers.rect_oracle(oracle, rt, rn, rl, qt, qn, ql, K, KSPACE21)
        counts = np.zeros(numer.shape, dtype=abi.COUNTS_DTYPE)
        counts["numer"], counts["denom"] = numer, denom
        shares = helpers.shares_a_hash(rt, rn, qt, qn, s)
        assert (qn == 0).any() and (numer >= 1).any() and not shares[0].any() and not shares[3].any()
        out.append({"sq": sq, "rt": rt, "rn": rn, "rl": rl, "qt": qt, "qn": qn, "ql": ql, "counts": counts, "shares": shares})
    return out


@pytest.mark.parametrize("form", list(FORMS))
def test_merge_form_on_the_rect_table(eng, rect_cases, merge_form, capfd, form):
    """queries located in the reference table's index: values below every table value, above, between two, equal to a value one
    row holds or many, an empty query, reference rows that are copies (the columns' representatives), three query sketch sizes"""
    merge_form(form)
    for c in rect_cases:
        ref, qry = eng.table_upload(c["rt"], c["rn"], c["rl"]), eng.table_upload(c["qt"], c["qn"], c["ql"])
        nq = len(c["qn"])
        try:
            for qb, qe in ((0, nq), (3, nq - 2)):
                capfd.readouterr()
                got = eng.compare_rect_host(ref, qry, qb, qe)
                lines = _merge_lines(capfd.readouterr().err)
                want = c["counts"][qb:qe]
                bad = np.argwhere((got["numer"] != want["numer"]) | (got["denom"] != want["denom"]))
                assert len(bad) == 0, (form, c["sq"], qb, qe, [(int(q) + qb, int(r), tuple(got[q, r]), tuple(want[q, r])) for q, r in bad[:5]])
                assert got.tobytes() == np.ascontiguousarray(want).tobytes()
                assert lines == [(form, int(c["shares"][qb:qe].sum()), False)], (form, c["sq"], qb, qe, lines)
                _same_as_the_other_forms(("rect", c["sq"], qb, qe), got)
        finally:
            ref.free()
            qry.free()


def _survivors(c, host, max_d, max_p):
    """the oracle's passing pairs of the whole triangle, reference order, as mg_result records with the host finish's doubles"""
    at = np.nonzero(_oracle_pass(c, max_d, max_p))[0]
    rows, cols = helpers.tri_rows_cols(0, c["n"])
    want = np.zeros(len(at), dtype=abi.RESULT_DTYPE)
    want["row"], want["col"] = rows[at], cols[at]
    want["numer"], want["denom"] = c["numer"][at], c["denom"][at]
    want["distance"], want["p_value"] = host["distance"][at], host["p_value"][at]
    assert np.all(host["pass"][at] == 1) and int(host["pass"].sum()) == len(at)
    return want


@pytest.mark.parametrize("form", ["lanes", "pack 43"])
@pytest.mark.parametrize("table", ["sizes", "pack"])
def test_merge_form_feeds_the_list_path(eng, oracle, cases, merge_form, capfd, table, form):
    """a thresholded job and the matrix of exceptions take the candidates as LISTS: the job is set, nothing is scattered, and
    sp_row_counts / sp_gather_rows (and, for the exceptions, sp_edges_*) put the merge's results in reference order.  The list
    engine leaves a table with an empty or a copied row to the matrix path (host_compare.cpp: open_index), so `sizes` runs as it
    is -- its answer must be right whichever route serves it -- and once more without its empty rows, where the lists must be
    what ran."""
    merge_form(form)
    max_d, max_p = 0.5, -1.0                                # distance 1 (no common hash) fails, every pair that shares passes or not by its own count
    todo = [(c, None) for c in cases(table) if c["s"] in (8, 33, 300)]
    if table == "sizes":
        rng = np.random.default_rng(7)
        todo += [(_tri_case(oracle, [r for r in c["rows"] if r], c["s"], rng), True) for c, _ in list(todo)]
    for c, must_list in todo:
        plain = all(len(r) for r in c["rows"]) and len({tuple(r) for r in c["rows"]}) == c["n"]      # no empty row, no copy
        assert must_list is None or plain
        tab = eng.table_upload(c["table"], c["nhash"], c["lengths"])
        try:
            fin = eng.finish_tri(c["counts"], c["lengths"], 0, c["n"], K, KSPACE21, max_d, max_p)
            _check_records_against_oracle(fin, c, 0, len(fin), max_d, max_p)
            want = _survivors(c, fin, max_d, max_p)
            assert 0 < len(want) < len(fin)
            capfd.readouterr()
            got = eng.compare_tri_results(tab, K, KSPACE21, max_d, max_p)
            lines = _merge_lines(capfd.readouterr().err)
            assert np.array_equal(got["row"], want["row"]) and np.array_equal(got["col"], want["col"]), (table, c["s"], form)
            assert got.tobytes() == want.tobytes(), (table, c["s"], form)
            cand = int(c["shares"].sum())
            if plain:
                assert lines == [(form, cand, True)], (table, c["s"], form, lines)
            else:
                assert lines and all(l[0] == form for l in lines), (table, c["s"], form, lines)
            capfd.readouterr()
            edges = eng.compare_tri_sparse(tab)
            lines = _merge_lines(capfd.readouterr().err)
            assert edges.tobytes() == helpers.edges_of_tri(c["numer"], c["denom"], 0, c["n"]).tobytes(), (table, c["s"], form)
            if plain:
                assert lines == [(form, cand, True)], (table, c["s"], form, lines)
        finally:
            tab.free()
