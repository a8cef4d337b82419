"""`mash triangle -N`: what is refused is refused before a device is opened (exit status 1 and the message, on a machine without a GPU)."""
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


@pytest.mark.parametrize("n", ["0", "1025", "2.5", "x"])
def test_nearest_refuses_counts_outside_its_range(built, n):
    r = run("triangle", "-N", n, "g1.fa", "g3.fa")
    assert r.returncode == 1 and r.stdout == ""
    assert r.stderr == f"ERROR: Argument to -N must be an integer between 1 and 1024 ({n} given)\n"


def test_usage_lists_nearest(built):
    r = run("triangle", "-h")
    assert r.returncode == 0 and "-N <int>" in r.stdout and "Implies -E" in r.stdout
