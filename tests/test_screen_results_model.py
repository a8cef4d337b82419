"""The tail of `mash screen` on the CPU: the pure-Python model (tests/screen_results_model.py) against the recorded stdout
of the REFERENCE CLI (tests/golden/screen_results, written by tests/golden/make_screen_results_golden.py).

The model is the specification the GPU tests of mg_screen_results_host are judged by; that it reproduces the reference
byte for byte on every parity fixture -- the %g columns, the winner reallocation with its length rule, the upper median,
both filters -- is the evidence that it reads the reference correctly.  One fixture (`full_tie`) is excluded from byte
parity: one genome sketched under two names, where the reference gives each hash to whichever name its unordered_set
lists first.  Hashes and pool k-mers come from the CPU oracle; the p-value from the exported host function
mg_p_value_within (pinned by test_pvalue_exact.py)."""
import json, os

import pytest

import screen_results_model as model

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "screen_results")
IN = os.path.join(GOLD, "in")
CASES = json.load(open(os.path.join(GOLD, "cases.json")))["screen"]
PARITY = [c for c in CASES if c["parity"]]
EXCLUDED = [c for c in CASES if not c["parity"]]


def test_only_the_full_tie_is_excluded_from_parity():
    assert [c["name"] for c in EXCLUDED] == ["full_tie"]
    want = {"plain", "winner", "identity", "pvalue", "all_rows", "winner_filters", "two_files", "stdin", "clade_winner", "length_rule",
            "short_sketch", "protein"}
    assert want <= {c["name"] for c in PARITY}


@pytest.mark.parametrize("case", PARITY, ids=[c["name"] for c in PARITY])
def test_model_prints_what_the_reference_printed(oracle, case):
    want = open(os.path.join(GOLD, case["name"] + ".out"), "rb").read()
    assert want.count(b"\n") >= 2
    assert model.case_lines(oracle, case, IN) == want


def test_fixtures_pin_what_they_are_meant_to(oracle):
    out = {c["name"]: open(os.path.join(GOLD, c["name"] + ".out")).read().splitlines() for c in CASES}
    assert len(out["identity"]) < len(out["plain"]) and len(out["pvalue"]) < len(out["k11_plain"])          # the filters bite
    assert any(ln.split("\t")[1].startswith("0/") for ln in out["all_rows"])                                # -i -1 prints shared == 0
    assert out["winner"] != out["plain"]
    took = [int(ln.split("\t")[1].split("/")[0]) for ln in out["length_rule"]]
    assert took[:2] == [0, 0] and took[2] > 100                                                             # the longer copy takes all
    assert any(int(ln.split("\t")[1].split("/")[1]) < 1000 for ln in out["short_sketch"])                   # denom < s
    # the clade: most observed hashes have several holders
    case = next(c for c in CASES if c["name"] == "clade_winner")
    _, _, _, rows, observed, _ = model.fixture_inputs(oracle, case, IN)
    holders = {}
    for i, r in enumerate(rows):
        for h in r:
            if int(h) in observed:
                holders.setdefault(int(h), []).append(i)
    assert sum(1 for v in holders.values() if len(v) > 1) > len(holders) / 2


def test_full_tie_differs_at_most_in_the_name_that_carries_the_hashes(oracle):
    (case,) = EXCLUDED
    ref = [ln.split("\t") for ln in open(os.path.join(GOLD, case["name"] + ".out")).read().splitlines()]
    got = [ln.split("\t") for ln in model.case_lines(oracle, case, IN).decode().splitlines()]
    assert [f[4] for f in got] == [f[4] for f in ref] == ["first", "second", "third"]
    assert got[2] == ref[2]
    total = lambda rows: sum(int(f[1].split("/")[0]) for f in rows[:2])
    assert total(got) == total(ref) > 100
    assert got[0][1] == "%d/200" % total(got) and got[1][1] == "0/200"                      # the model decides: lowest row


# ---- the model's own rules on hand-made hits
def test_winner_rules_small():
    P = lambda x, ss, ks, d: 0.5
    nhash, lengths = [4, 4, 4, 2], [100, 200, 200, 50]
    # hash 1: rows 0 1 2; hash 2: rows 0 1; hash 3: rows 1 2; hash 4: row 3 alone
    hits = [(0, 5, 1), (1, 5, 1), (2, 5, 1), (0, 7, 2), (1, 7, 2), (1, 2, 3), (2, 2, 3), (3, 9, 4)]
    plain = model.results(hits, nhash, lengths, 21, 1000, 4.0 ** 21, p_value=P)
    assert [(r[0], r[1], r[2], r[3]) for r in plain] == [(0, 2, 4, 7), (1, 3, 4, 5), (2, 2, 4, 5), (3, 1, 2, 9)]
    won = model.results(hits, nhash, lengths, 21, 1000, 4.0 ** 21, winner=True, p_value=P)
    assert [(r[0], r[1], r[3]) for r in won] == [(1, 3, 5), (3, 1, 9)]           # row 1 has the best score everywhere it holds
    # equal scores: length decides, then the lower row
    hits = [(0, 1, 1), (1, 1, 1), (2, 1, 1)]
    won = model.results(hits, [4, 4, 4], [100, 200, 200], 21, 1000, 4.0 ** 21, winner=True, min_identity=-1.0, p_value=P)
    assert [(r[0], r[1]) for r in won] == [(0, 0), (1, 1), (2, 0)]
    assert won[0][4] == 0.0 and won[0][5] == 1.0 and won[0][3] == 0


def test_upper_median_and_identity():
    P = lambda x, ss, ks, d: 0.0
    hits = [(0, c, h) for h, c in enumerate([9, 1, 5, 3])]
    (r,) = model.results(hits, [10], [1], 21, 1, 1.0, p_value=P)
    assert r[3] == 5 and r[4] == (4 / 10) ** (1 / 21)
    assert model.identity(0, 0, 21) == 1.0 and model.identity(7, 7, 21) == 1.0 and model.identity(0, 7, 21) == 0.0
    assert model.set_size([]) == 0 and model.set_size([1 << 62, 1 << 63]) == 4
