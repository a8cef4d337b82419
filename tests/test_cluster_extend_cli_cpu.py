"""`mash cluster -A`: what is refused is refused before a device is opened (exit status 1, one ERROR line, empty stdout, on a machine
without a GPU) -- a missing file, a directory in its place, a line without two tabs, a cluster number that is not a positive
integer, -A together with -T; the usage text of `mash cluster` and the top-level command list name -A."""
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


def refused(r):
    assert r.returncode == 1 and r.stdout == ""
    assert r.stderr.startswith("ERROR: ") and r.stderr.endswith("\n") and r.stderr.count("\n") == 1, r.stderr
    return r.stderr


def test_a_missing_file_is_refused(built, tmp_path):
    gone = str(tmp_path / "no such file")
    for opts in ((), ("-R",), ("-d", "0.1", "-C")):
        assert refused(run("cluster", "-A", gone, *opts, "g1.fa", "g3.fa")) == f"ERROR: Could not open {gone} for reading.\n"
    assert "ERROR: Could not" in refused(run("cluster", "-A", str(tmp_path), "g1.fa", "g3.fa"))      # a directory: nothing to read
    assert refused(run("cluster", "g1.fa", "g3.fa", "-A")) == "ERROR: -A requires an argument\n"


@pytest.mark.parametrize("text, line", [("1\t1\n", 1), ("1\t1\tg1\n2 1 g3\n", 2), ("1\t1\tg1\n\n2\t1\tg3\n", 2), ("g1\n", 1)])
def test_a_line_without_two_tabs_is_refused(built, tmp_path, text, line):
    f = tmp_path / "old"
    f.write_text(text)
    assert refused(run("cluster", "-A", str(f), "g1.fa", "g3.fa")) == \
        f"ERROR: Line {line} of {f} is not a line of `mash cluster` (number, size and ID between tabs).\n"


@pytest.mark.parametrize("number", ["0", "-1", "1.5", "x", "", " 1", "1e3", "99999999999999999999999"])
def test_a_number_that_is_not_a_positive_integer_is_refused(built, tmp_path, number):
    f = tmp_path / "old"
    f.write_text(f"1\t1\tg1\n{number}\t1\tg3\n")
    for opts in ((), ("-R",)):
        assert refused(run("cluster", "-A", str(f), *opts, "g1.fa", "g3.fa")) == \
            f"ERROR: Line 2 of {f} does not begin with a cluster number (a positive integer).\n"


@pytest.mark.parametrize("opts", [("-T",), ("-d", "0.03", "-T"), ("-T", "-d", "1", "-v", "1")])
def test_a_with_t_is_refused(built, tmp_path, opts):
    f = tmp_path / "old"
    f.write_text("1\t1\tg1\n")
    assert refused(run("cluster", "-A", str(f), *opts, "g1.fa", "g3.fa")) == "ERROR: -T and -A cannot be given together.\n"
    assert refused(run("cluster", *opts, "-A", str(tmp_path / "gone"), "g1.fa", "g3.fa")) == "ERROR: -T and -A cannot be given together.\n"


def test_cluster_usage_names_a(built):
    for args in (("cluster", "-h"), ("cluster",), ("cluster", "-A", "x", "-h")):
        r = run(*args)
        assert r.returncode == 0 and r.stderr == ""
        assert "\n  -A <file> " in r.stdout and "earlier" in r.stdout and "are not checked" in r.stdout and "Not with -T" in r.stdout
        assert "\n  -T  " in r.stdout and "\n  -R  " in r.stdout and "-d <num>" in r.stdout and "[0.05]" in r.stdout     # what was there stays


def test_top_level_usage_names_a(built):
    r = subprocess.run([MASH], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "\n  cluster   " in r.stdout and "(-A)" in r.stdout and "(-T)" in r.stdout and "(-R)" in r.stdout
