"""The judge of tests/test_rect_gpu.py, checked on the CPU: helpers.rect_oracle (a rect job read out of the oracle's triangle of
the stacked tables, both cut to the smaller sketch size) against oracle.compare on the rows as they are, pair by pair, and
helpers.expand_rect (the rule of mg_compare_rect_sparse_host, include/mashgpu.h) against the full result -- at equal and
unequal sketch sizes.  Then the conditions the GPU tests' tables must meet, on the oracle's output alone."""
import numpy as np
import pytest

from tests import helpers
from workloads import synth

KSPACE21 = 4.0 ** 21


def _case(s_ref, s_qry):
    """40 x 9 rows as in test_compare_rect_with_different_sketch_sizes: a short query, a query equal to (a prefix of) a
    reference, and besides an empty query and a reference with one hash"""
    n_ref, n_qry = 40, 9
    big = max(s_ref, s_qry)
    table, nhash, _ = synth.clustered_sketches(n_ref + n_qry, big, clusters=3, seed=s_ref + s_qry, pool=int(1.5 * big), private=int(0.4 * big))
    lengths = np.random.default_rng(s_ref).integers(10 ** 4, 10 ** 8, n_ref + n_qry).astype(np.uint64)
    rt = np.full((n_ref, s_ref), helpers.PAD, dtype=np.uint64)
    qt = np.full((n_qry, s_qry), helpers.PAD, dtype=np.uint64)
    rn = np.minimum(nhash[:n_ref], s_ref).astype(np.uint32)
    qn = np.minimum(nhash[n_ref:], s_qry).astype(np.uint32)
    qn[2] = s_qry // 5
    qn[6] = 0
    rn[5] = 1
    for i in range(n_ref):
        rt[i, : rn[i]] = table[i, : rn[i]]
    for i in range(n_qry):
        qt[i, : qn[i]] = table[n_ref + i, : qn[i]]
    qn[4] = min(s_qry, rn[7])
    qt[4] = helpers.PAD
    qt[4, : qn[4]] = rt[7, : qn[4]]
    return rt, rn, lengths[:n_ref], qt, qn, lengths[n_ref:]


@pytest.mark.parametrize("s_ref,s_qry", [(256, 128), (128, 256), (256, 256)])
def test_rect_oracle_equals_compare_on_the_untruncated_rows(oracle, s_ref, s_qry):
    rt, rn, rl, qt, qn, ql = _case(s_ref, s_qry)
    numer, denom, dist, pval = helpers.rect_oracle(oracle, rt, rn, rl, qt, qn, ql, 21, KSPACE21)
    assert numer.shape == (9, 40) and numer.dtype == np.uint32
    s = min(s_ref, s_qry)
    for q in range(9):
        for r in range(40):
            o = oracle.compare(rt[r, : rn[r]], qt[q, : qn[q]], int(rl[r]), int(ql[q]), s, 21, KSPACE21)
            assert (int(numer[q, r]), int(denom[q, r])) == (o.numer, o.denom), (q, r)
            assert dist[q, r] == o.distance and pval[q, r] == o.p_value, (q, r)
    assert numer[4, 7] == denom[4, 7] == min(int(qn[4]), s)                     # the copy finds its original
    assert (numer == 0).any() and (numer > 0).any()
    # the rule and the exceptions give the whole result, unequal sizes included; so does a range of queries
    full = np.zeros(numer.shape, dtype=helpers.COUNTS)
    full["numer"], full["denom"] = numer, denom
    edges = helpers.edges_of(numer, denom)
    assert 0 < len(edges) < numer.size
    assert helpers.expand_rect(edges, rn, qn, s, 0, 9, 40).tobytes() == full.tobytes()
    part = helpers.edges_of(numer[3:8], denom[3:8], 3)
    assert helpers.expand_rect(part, rn, qn, s, 3, 8, 40).tobytes() == full[3:8].tobytes()
    assert helpers.expand_rect(part[:0], rn, qn, s, 9, 9, 40).shape == (0, 40)


@pytest.mark.parametrize("name", ["clean", "ragged", "species"])
def test_rect_tables_meet_their_conditions(oracle, name):
    case = getattr(helpers, "rect_case_" + name)()
    numer, denom, _, _ = helpers.rect_case_oracle(oracle, case)
    helpers.check_rect_case_conditions(name, case, numer, denom)
    if name == "species":
        return
    # the rule holds for every numer-0 pair at unequal sizes too
    for s_ref, s_qry in ((256, 128), (128, 256)):
        sized = helpers.rect_case_sized(case, s_ref, s_qry)
        n2, d2, _, _ = helpers.rect_case_oracle(oracle, sized)
        full = np.zeros(n2.shape, dtype=helpers.COUNTS)
        full["numer"], full["denom"] = n2, d2
        got = helpers.expand_rect(helpers.edges_of(n2, d2), sized["rn"], sized["qn"], 128, 0, len(sized["qn"]), len(sized["rn"]))
        assert got.tobytes() == full.tobytes()
        assert (n2 >= 1).any() and not np.array_equal(n2, numer)
