"""`mash cluster`: which combinations of -R, -B, -T, -A and -M are refused, with which line, over all 32 subsets.  A refusal comes
before the -A file is read and before a device is opened (exit status 1, nothing on stdout and exactly one ERROR line, on a machine
without a GPU); where two refusals apply, the first of the command's ordered list is the one printed.  The eight subsets that are
allowed need a device and are not run here, but `-d 1 -v 1` is refused on each of them, again before any device."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASH = os.path.join(ROOT, "mash_amd", "bin", "mash")
IN = os.path.join(ROOT, "tests", "golden", "cli", "in")

FLAGS = ("-R", "-B", "-T", "-A", "-M")
SUBSETS = [s for k in range(len(FLAGS) + 1) for s in itertools.combinations(FLAGS, k)]
ALLOWED = [(), ("-R",), ("-B",), ("-R", "-B"), ("-T",), ("-A",), ("-R", "-A"), ("-M",)]
REASON = {("-M", "-A"): " (the weights between earlier inputs are not among the pairs -A compares)",
          ("-B", "-A"): " (a new representative can be nearer to an earlier member)"}


def expected(subset):
    """the command's precedence, restated: the first pair of this list that the subset holds is the one named; None: allowed"""
    for pair in (("-M", "-R"), ("-M", "-B"), ("-M", "-T"), ("-M", "-A"), ("-B", "-T"), ("-B", "-A"), ("-T", "-R"), ("-T", "-A")):
        if pair[0] in subset and pair[1] in subset:
            return f"ERROR: {pair[0]} and {pair[1]} cannot be given together{REASON.get(pair, '')}.\n"
    return None


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
    """the option lists of a subset: with -A, one with an existing file and one with a missing one"""
    if "-A" not in subset:
        return [list(subset)]
    earlier = tmp_path / "earlier.tsv"
    earlier.write_text("1\t1\tg1.fa\n")
    return [[a for o in subset for a in ((o, str(f)) if o == "-A" else (o,))] for f in (earlier, tmp_path / "no such file")]


def test_the_allowed_subsets_are_the_eight():
    assert sorted(s for s in SUBSETS if expected(s) is None) == sorted(ALLOWED)
    assert len(SUBSETS) == 32 and len(set(SUBSETS)) == 32


@pytest.mark.parametrize("subset", [s for s in SUBSETS if expected(s) is not None], ids=lambda s: "".join(s))
def test_refused_subset(built, tmp_path, subset):
    for opts in forms(subset, tmp_path):
        r = run("cluster", *opts, "g1.fa", "g3.fa")
        assert one_error_line(r), (opts, r.stderr)
        assert r.stderr == expected(subset), (opts, r.stderr)


@pytest.mark.parametrize("subset", ALLOWED, ids=lambda s: "".join(s) or "plain")
def test_every_pair_an_edge_is_refused_on_allowed_subset(built, tmp_path, subset):
    for opts in forms(subset, tmp_path):
        r = run("cluster", *opts, "-d", "1", "-v", "1", "g1.fa", "g3.fa")
        assert one_error_line(r), (opts, r.stderr)
        assert r.stderr == "ERROR: With -d 1 and -v 1 every pair is an edge; give a smaller maximum.\n", (opts, r.stderr)
