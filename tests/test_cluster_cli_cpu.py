"""`mash cluster`: what is refused is refused before a device is opened (exit status 1 and one ERROR line, on a machine without
a GPU); the usage text names the -d default; the top-level usage lists the command."""
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


@pytest.mark.parametrize("opts", [("-d", "1", "-v", "1"), ("-v", "1", "-d", "1.0")])
def test_cluster_refuses_both_filters_off(built, opts):
    r = run("cluster", *opts, "g1.fa", "g3.fa")
    assert r.returncode == 1 and r.stdout == ""
    assert r.stderr == "ERROR: With -d 1 and -v 1 every pair is an edge; give a smaller maximum.\n"


@pytest.mark.parametrize("opt,val", [("-d", "1.5"), ("-d", "x"), ("-v", "-0.1")])
def test_cluster_refuses_filters_outside_their_range(built, opt, val):
    r = run("cluster", opt, val, "g1.fa", "g3.fa")
    assert r.returncode == 1 and r.stdout == ""
    assert r.stderr == f"ERROR: Argument to {opt} must be a number between 0 and 1 ({val} given)\n"


def test_cluster_usage_names_the_defaults(built):
    for args in (("cluster", "-h"), ("cluster",)):
        r = run(*args)
        assert r.returncode == 0 and r.stderr == ""
        assert "mash cluster [options] <seq1> [<seq2>] ..." in r.stdout
        assert "-d <num>" in r.stdout and "[0.05]" in r.stdout and "-v <num>" in r.stdout and "[1.0]" in r.stdout


def test_top_level_usage_lists_cluster(built):
    r = subprocess.run([MASH], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "\n  cluster   " in r.stdout
