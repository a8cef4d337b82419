"""`mash cluster -T`: what is refused is refused before a device is opened (exit status 1 and one ERROR line, on a machine without a
GPU) -- -T together with -R, both filters off, a filter outside its range; the usage text of `mash cluster` and the top-level command
list name the minimum spanning forest."""
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


@pytest.mark.parametrize("opts", [("-T", "-R"), ("-R", "-d", "0.03", "-T"), ("-T", "-R", "-d", "1", "-v", "1")])
def test_cluster_t_with_r_is_refused(built, opts):
    r = run("cluster", *opts, "g1.fa", "g3.fa")
    assert r.returncode == 1 and r.stdout == ""
    assert r.stderr == "ERROR: -T and -R cannot be given together.\n"


@pytest.mark.parametrize("opts", [("-T", "-d", "1", "-v", "1"), ("-v", "1", "-d", "1.0", "-T")])
def test_cluster_t_refuses_both_filters_off(built, opts):
    r = run("cluster", *opts, "g1.fa", "g3.fa")
    assert r.returncode == 1 and r.stdout == ""
    assert r.stderr == "ERROR: With -d 1 and -v 1 every pair is an edge; give a smaller maximum.\n"


def test_cluster_t_refuses_a_filter_outside_its_range(built):
    r = run("cluster", "-T", "-d", "1.5", "g1.fa", "g3.fa")
    assert r.returncode == 1 and r.stdout == ""
    assert r.stderr == "ERROR: Argument to -d must be a number between 0 and 1 (1.5 given)\n"
    r = run("cluster", "-T", "-v", "-0.5", "g1.fa", "g3.fa")
    assert r.returncode == 1 and r.stdout == "" and r.stderr.startswith("ERROR: ")


def test_cluster_usage_names_t(built):
    for args in (("cluster", "-h"), ("cluster",), ("cluster", "-T", "-h")):
        r = run(*args)
        assert r.returncode == 0 and r.stderr == ""
        assert "\n  -T  " in r.stdout and "minimum spanning forest" in r.stdout and "Not with -R" in r.stdout
        assert "\n  -R  " in r.stdout and "-d <num>" in r.stdout and "[0.05]" in r.stdout     # what was there stays


def test_top_level_usage_names_the_forest(built):
    r = subprocess.run([MASH], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "\n  cluster   " in r.stdout and "(-T)" in r.stdout and "(-R)" in r.stdout
