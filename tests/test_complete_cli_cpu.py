"""`mash cluster -L` with the older flags: -L is refused with each of -R, -B, -M, -T and -A, over all 31 subsets of them that are not
empty (-L alone needs a device and is not run here).  The refusal names the first pair of the command's ordered list that the
subset holds -- the eight older rows come first, then -L with -R, -B, -M, -T, -A in that order -- and comes before the -A file is
read and before a device is opened: exit status 1, nothing on stdout and exactly one ERROR line, on a machine without a GPU.
`-L -d 1 -v 1` is refused as on every other form."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASH = os.path.join(ROOT, "mash_amd", "bin", "mash")
IN = os.path.join(ROOT, "tests", "golden", "cli", "in")

OLD = ("-R", "-B", "-T", "-A", "-M")
SUBSETS = [s for k in range(1, len(OLD) + 1) for s in itertools.combinations(OLD, k)]
REASON = {("-M", "-A"): " (the weights between earlier inputs are not among the pairs -A compares)",
          ("-B", "-A"): " (a new representative can be nearer to an earlier member)"}
ORDER = (("-M", "-R"), ("-M", "-B"), ("-M", "-T"), ("-M", "-A"), ("-B", "-T"), ("-B", "-A"), ("-T", "-R"), ("-T", "-A"),
         ("-L", "-R"), ("-L", "-B"), ("-L", "-M"), ("-L", "-T"), ("-L", "-A"))


def expected(subset):
    """the command's precedence, restated: the first pair of ORDER that -L and the subset hold"""
    given = ("-L",) + tuple(subset)
    for pair in ORDER:
        if pair[0] in given and pair[1] in given:
            return f"ERROR: {pair[0]} and {pair[1]} cannot be given together{REASON.get(pair, '')}.\n"
    raise AssertionError("-L with an older flag is always refused")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    if not os.path.exists(MASH):
        g.build()
    return True


def run(*args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")       # no device, wherever this runs
    return subprocess.run([MASH, *args], capture_output=True, text=True, cwd=IN, env=env, timeout=120)


def one_error_line(r):
    return r.returncode == 1 and r.stdout == "" and r.stderr.count("\n") == 1 and r.stderr.startswith("ERROR: ")


def forms(subset, tmp_path):
    """the option lists of -L with a subset, -L first and last: with -A, one with an existing file and one with a missing one"""
    files = [None]
    if "-A" in subset:
        earlier = tmp_path / "earlier.tsv"
        earlier.write_text("1\t1\tg1.fa\n")
        files = [earlier, tmp_path / "no such file"]
    out = []
    for f in files:
        opts = [a for o in subset for a in ((o, str(f)) if o == "-A" else (o,))]
        out += [["-L", *opts], [*opts, "-L"]]
    return out


def test_the_subsets_are_the_31_and_the_single_flags_name_themselves():
    assert len(SUBSETS) == 31 and len(set(SUBSETS)) == 31
    for flag in OLD:
        assert expected((flag,)) == f"ERROR: -L and {flag} cannot be given together.\n"
    assert expected(("-R", "-B")) == "ERROR: -L and -R cannot be given together.\n"          # allowed together without -L
    assert expected(("-T", "-A")) == "ERROR: -T and -A cannot be given together.\n"          # an older row comes first


@pytest.mark.parametrize("subset", SUBSETS, ids=lambda s: "-L" + "".join(s))
def test_refused_with_an_older_flag(built, tmp_path, subset):
    for opts in forms(subset, tmp_path):
        r = run("cluster", *opts, "g1.fa", "g3.fa")
        assert one_error_line(r), (opts, r.stderr)
        assert r.stderr == expected(subset), (opts, r.stderr)


def test_every_pair_an_edge_is_refused(built):
    for opts in (["-L", "-d", "1", "-v", "1"], ["-L", "-d", "1"], ["-d", "1", "-v", "1", "-L", "-C"]):
        r = run("cluster", *opts, "g1.fa", "g3.fa")
        assert one_error_line(r), (opts, r.stderr)
        assert r.stderr == "ERROR: With -d 1 and -v 1 every pair is an edge; give a smaller maximum.\n", (opts, r.stderr)


def test_help_names_the_option(built):
    r = run("cluster", "-h")
    assert r.returncode == 0 and "  -L        Complete-linkage clusters" in r.stdout
    assert "-L" in run().stdout + run().stderr
