"""`mash within`: usage and what is refused before a device is opened (on a machine without a GPU)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASH = os.path.join(ROOT, "mash_amd", "bin", "mash")
IN = os.path.join(ROOT, "tests", "golden", "within")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    if not os.path.exists(MASH):
        g.build()
    return True


def run(*args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")       # no device, wherever this runs
    return subprocess.run([MASH, *args], capture_output=True, text=True, cwd=IN, env=env, timeout=120)


def test_help_prints_usage(built):
    r = run("within", "-h")
    assert r.returncode == 0 and r.stderr == ""
    assert "mash within [options] <reference> <query> [<query>] ..." in r.stdout and "-e <num>" in r.stdout
    assert "[score, error-bound, reference-ID, query-ID]" in r.stdout


@pytest.mark.parametrize("args", [[], ["ref.fa.gz"], ["-e", "0.3", "ref.fa.gz"]])
def test_fewer_than_two_arguments_print_usage_and_exit_0(built, args):
    r = run("within", *args)                                                       # CommandContain.cpp:35-39
    assert r.returncode == 0 and r.stdout == run("within", "-h").stdout


def test_command_table_lists_within(built):
    r = run()
    assert r.returncode == 0 and "\n  within    Estimate the containment of query sequences within references.\n" in r.stdout


@pytest.mark.parametrize("e", ["x", "e5", "--3"])
def test_bad_error_threshold_is_refused(built, e):
    r = run("within", "-e", e, "ref.fa.gz", "queries.fa.gz")
    assert r.returncode == 1 and r.stdout == ""
    assert r.stderr == f"ERROR: Argument to -e must be a number ({e} given)\n"


def test_missing_error_threshold_argument(built):
    r = run("within", "ref.fa.gz", "queries.fa.gz", "-e")
    assert r.returncode == 1 and r.stdout == "" and r.stderr == "ERROR: -e requires an argument\n"


@pytest.mark.parametrize("opt,letter", [(["-k", "16"], "k"), (["-n"], "n")])
def test_sketch_reference_refuses_what_it_fixes_itself(built, opt, letter):
    r = run("within", *opt, "ref_s1000.msh", "queries.fa.gz")                     # CommandContain.cpp:61-71
    assert r.returncode == 1 and r.stdout == ""
    assert r.stderr == f"ERROR: The option -{letter} cannot be used when a sketch is provided; it is inherited from the sketch.\n"
