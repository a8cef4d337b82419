"""`mash cluster -B`: what is refused is refused before a device is opened (exit status 1, nothing on stdout and exactly one ERROR
line, on a machine without a GPU): -B with -T, -B with -A, and what -R refuses; the usage text names -B, the nearest
representative and the fourth output field, and the top-level command list names it."""
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


@pytest.mark.parametrize("opts", [("-B", "-T"), ("-T", "-B", "-d", "0.1"), ("-R", "-B", "-T")])
def test_cluster_b_refuses_t(built, opts):
    r = run("cluster", *opts, "g1.fa", "g3.fa")
    assert one_error_line(r), r.stderr
    assert r.stderr == "ERROR: -B and -T cannot be given together.\n"


@pytest.mark.parametrize("opts", [("-B",), ("-R", "-B")])
def test_cluster_b_refuses_a(built, opts, tmp_path):
    earlier = tmp_path / "earlier.tsv"
    earlier.write_text("1\t1\tg1.fa\n")
    r = run("cluster", *opts, "-A", str(earlier), "g1.fa", "g3.fa")
    assert one_error_line(r), r.stderr
    assert r.stderr.startswith("ERROR: -B and -A cannot be given together")
    r = run("cluster", *opts, "-A", str(tmp_path / "no such file"), "g1.fa", "g3.fa")      # refused before the file is looked at
    assert one_error_line(r) and r.stderr.startswith("ERROR: -B and -A cannot be given together"), r.stderr


def test_cluster_b_refuses_what_r_refuses(built):
    r = run("cluster", "-B", "-d", "1", "-v", "1", "g1.fa", "g3.fa")
    assert one_error_line(r) and r.stderr == "ERROR: With -d 1 and -v 1 every pair is an edge; give a smaller maximum.\n"


def test_cluster_usage_names_b(built):
    for args in (("cluster", "-h"), ("cluster",), ("cluster", "-B", "-h")):
        r = run(*args)
        assert r.returncode == 0 and r.stderr == ""
        assert "\n  -B  " in r.stdout and "nearest representative" in r.stdout
        assert "fourth field" in r.stdout and "representative-ID" in r.stdout
        assert "Not with -A" in r.stdout.replace("\n            ", " ")
        assert "\n  -R  " in r.stdout and "first representative" in r.stdout and "-d <num>" in r.stdout and "[0.05]" in r.stdout


def test_top_level_usage_names_b(built):
    r = subprocess.run([MASH], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "\n  cluster   " in r.stdout and "(-B)" in r.stdout and "(-R)" in r.stdout
