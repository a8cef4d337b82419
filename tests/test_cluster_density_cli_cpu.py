"""`mash cluster -D`: what is refused is refused before a device is opened (exit status 1, nothing on stdout and exactly one ERROR
line, on a machine without a GPU): -D with each of -R, -B, -T, -A, -M and -L, an argument outside 1 .. 2^31 - 1 or no number, and
-d 1 -v 1; the usage text names -D, its roles and its two extra fields, and the top-level command list names it."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASH = os.path.join(ROOT, "mash_amd", "bin", "mash")
IN = os.path.join(ROOT, "tests", "golden", "cli", "in")


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


@pytest.mark.parametrize("other", ["-R", "-B", "-T", "-M", "-L"])
def test_cluster_d_refuses_the_other_forms(built, other):
    for opts in (("-D", "3", other), (other, "-D", "3", "-d", "0.1")):
        r = run("cluster", *opts, "g1.fa", "g3.fa")
        assert one_error_line(r), r.stderr
        assert r.stderr == f"ERROR: -D and {other} cannot be given together.\n"


def test_cluster_d_refuses_a(built, tmp_path):
    earlier = tmp_path / "earlier.tsv"
    earlier.write_text("1\t1\tg1.fa\n")
    r = run("cluster", "-D", "3", "-A", str(earlier), "g1.fa", "g3.fa")
    assert one_error_line(r), r.stderr
    assert r.stderr.startswith("ERROR: -D and -A cannot be given together")
    r = run("cluster", "-D", "3", "-A", str(tmp_path / "no such file"), "g1.fa", "g3.fa")      # refused before the file is looked at
    assert one_error_line(r) and r.stderr.startswith("ERROR: -D and -A cannot be given together"), r.stderr


def test_earlier_refusals_keep_their_precedence(built):
    """the new rows stand behind the old ones: what was reported for a pair of the old options is still reported beside -D"""
    r = run("cluster", "-D", "3", "-M", "-R", "g1.fa", "g3.fa")
    assert one_error_line(r) and r.stderr == "ERROR: -M and -R cannot be given together.\n"
    r = run("cluster", "-D", "3", "-B", "-T", "g1.fa", "g3.fa")
    assert one_error_line(r) and r.stderr == "ERROR: -B and -T cannot be given together.\n"


@pytest.mark.parametrize("arg", ["0", "-3", "x", "2147483648", "4294967297", "1.5"])
def test_cluster_d_refuses_a_bad_count(built, arg):
    r = run("cluster", "-D", arg, "g1.fa", "g3.fa")
    assert one_error_line(r), r.stderr
    assert r.stderr.startswith("ERROR: Argument to -D must be an integer between 1 and 2") and f"({arg} given)" in r.stderr


def test_cluster_d_needs_an_argument(built):
    r = run("cluster", "g1.fa", "g3.fa", "-D")
    assert one_error_line(r) and r.stderr == "ERROR: -D requires an argument\n"


def test_cluster_d_refuses_every_pair_an_edge(built):
    r = run("cluster", "-D", "3", "-d", "1", "-v", "1", "g1.fa", "g3.fa")
    assert one_error_line(r) and r.stderr == "ERROR: With -d 1 and -v 1 every pair is an edge; give a smaller maximum.\n"


def test_cluster_usage_names_d(built):
    for args in (("cluster", "-h"), ("cluster",), ("cluster", "-D", "3", "-h")):
        r = run(*args)
        assert r.returncode == 0 and r.stderr == ""
        flat = r.stdout.replace("\n            ", " ")
        assert "\n  -D <int>  " in r.stdout and "Density clusters" in r.stdout and "minPts" in flat and "<int> + 1" in flat
        assert "[cluster-number, cluster-size, ID, role, neighbours]" in flat and "core, border or noise" in flat
        assert "Not with -R, -B, -T, -A, -M or -L" in flat
        assert "\n  -R  " in r.stdout and "\n  -L  " in r.stdout and "-d <num>" in r.stdout and "[0.05]" in r.stdout


def test_top_level_usage_names_d(built):
    r = subprocess.run([MASH], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "\n  cluster   " in r.stdout and "(-D)" in r.stdout and "(-L)" in r.stdout and "(-R)" in r.stdout
