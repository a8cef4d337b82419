"""`mash cluster -M`: what is refused is refused before a device is opened (exit status 1, nothing on stdout and exactly one ERROR
line, on a machine without a GPU): -M with -R, with -B, with -T and with -A; the usage text names -M, the medoid and the fourth
output field, and the top-level command list names it."""
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


@pytest.mark.parametrize("opts", [("-M", "-R"), ("-R", "-M", "-d", "0.1"), ("-M", "-R", "-B", "-T")])
def test_cluster_m_refuses_r(built, opts):
    r = run("cluster", *opts, "g1.fa", "g3.fa")
    assert one_error_line(r), r.stderr
    assert r.stderr == "ERROR: -M and -R cannot be given together.\n"


@pytest.mark.parametrize("opts", [("-M", "-B"), ("-B", "-M", "-C"), ("-M", "-B", "-T")])
def test_cluster_m_refuses_b(built, opts):
    r = run("cluster", *opts, "g1.fa", "g3.fa")
    assert one_error_line(r), r.stderr
    assert r.stderr == "ERROR: -M and -B cannot be given together.\n"


@pytest.mark.parametrize("opts", [("-M", "-T"), ("-T", "-M", "-d", "0.1")])
def test_cluster_m_refuses_t(built, opts):
    r = run("cluster", *opts, "g1.fa", "g3.fa")
    assert one_error_line(r), r.stderr
    assert r.stderr == "ERROR: -M and -T cannot be given together.\n"


def test_cluster_m_refuses_a(built, tmp_path):
    earlier = tmp_path / "earlier.tsv"
    earlier.write_text("1\t1\tg1.fa\n")
    want = "ERROR: -M and -A cannot be given together (the weights between earlier inputs are not among the pairs -A compares).\n"
    r = run("cluster", "-M", "-A", str(earlier), "g1.fa", "g3.fa")
    assert one_error_line(r) and r.stderr == want, r.stderr
    r = run("cluster", "-A", str(tmp_path / "no such file"), "-M", "g1.fa", "g3.fa")      # refused before the file is looked at
    assert one_error_line(r) and r.stderr == want, r.stderr


def test_cluster_m_refuses_what_plain_cluster_refuses(built):
    r = run("cluster", "-M", "-d", "1", "-v", "1", "g1.fa", "g3.fa")
    assert one_error_line(r) and r.stderr == "ERROR: With -d 1 and -v 1 every pair is an edge; give a smaller maximum.\n"


def test_cluster_usage_names_m(built):
    for args in (("cluster", "-h"), ("cluster",), ("cluster", "-M", "-h")):
        r = run(*args)
        assert r.returncode == 0 and r.stderr == ""
        flat = r.stdout.replace("\n            ", " ")
        assert "\n  -M  " in r.stdout and "medoid" in r.stdout and "medoid-ID" in r.stdout and "fourth field" in r.stdout
        assert "floor(shared * 2^32 / max(denominator, 1))" in flat and "equal scores to the earlier member" in flat
        assert "Not with -R, -B, -T or -A" in flat
        assert "\n  -R  " in r.stdout and "\n  -B  " in r.stdout and "-d <num>" in r.stdout and "[0.05]" in r.stdout


def test_top_level_usage_names_m(built):
    r = subprocess.run([MASH], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "\n  cluster   " in r.stdout and "(-M)" in r.stdout and "(-B)" in r.stdout and "(-R)" in r.stdout
