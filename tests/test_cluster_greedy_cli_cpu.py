"""`mash cluster -R`: what is refused is refused before a device is opened, with -R as without it (exit status 1 and one ERROR
line, on a machine without a GPU); the usage text and the top-level command list name the greedy representative clusters."""
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


@pytest.mark.parametrize("opts", [("-R", "-d", "1", "-v", "1"), ("-v", "1", "-d", "1.0", "-R")])
def test_cluster_r_refuses_both_filters_off(built, opts):
    r = run("cluster", *opts, "g1.fa", "g3.fa")
    assert r.returncode == 1 and r.stdout == ""
    assert r.stderr == "ERROR: With -d 1 and -v 1 every pair is an edge; give a smaller maximum.\n"


def test_cluster_r_refuses_a_filter_outside_its_range(built):
    r = run("cluster", "-R", "-d", "1.5", "g1.fa", "g3.fa")
    assert r.returncode == 1 and r.stdout == ""
    assert r.stderr == "ERROR: Argument to -d must be a number between 0 and 1 (1.5 given)\n"


def test_cluster_usage_names_r(built):
    for args in (("cluster", "-h"), ("cluster",), ("cluster", "-R", "-h")):
        r = run(*args)
        assert r.returncode == 0 and r.stderr == ""
        assert "\n  -R  " in r.stdout and "representative" in r.stdout and "first representative" in r.stdout
        assert "-d <num>" in r.stdout and "[0.05]" in r.stdout                   # what was there stays


def test_top_level_usage_names_representative_clusters(built):
    r = subprocess.run([MASH], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "\n  cluster   " in r.stdout and "(-R)" in r.stdout
