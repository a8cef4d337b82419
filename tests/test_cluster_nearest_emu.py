"""The kernels of `mash cluster -B`, unchanged, through their launchers on the CPU (tools/hipemu: work-items as fibers):
cf_append_kernel of mash_amd/csrc/cluster_forest.hip, the rounds of mash_amd/csrc/cluster_greedy.hip over the list with counts
(cg_round_edges_kernel<uint4>) and launch_nearest_assign (cg_rep_init_kernel, cn_key_kernel, cn_rep_kernel), against a sequential
C++ restatement that uses forest_before: a star whose centre is a representative in the MIDDLE of the index range (members below
it join it), a member between two representatives with the better one later and with the better one earlier, equal fractions
under different denominators (32/64 beside 16/32, 0/64 beside 0/0), a numer == 0 edge as a member's only edge, the band graph
whose answer has a closed form, lists whose length is not a multiple of 64, padding entries, lists that overflow and are regrown
(a first capacity of 1 edge, inside a word, one short, exactly enough), row blocks over one list, tables of 0 and 1 rows, and
random jobs with a fixed seed.  Every case also runs the list without counts (cg_append_kernel, cg_round_edges_kernel<uint2>,
cg_assign_kernel) and must still give the first representative of `mash cluster -R`, and the same states.
The emulator runs workgroups one after another: the races between workgroups on best_key[] and rep[] are exercised on the device
only (tests/test_cluster_nearest_gpu.py).  One small case also runs with work-items as OS threads under ThreadSanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emu", "cluster_nearest_emu_main.cpp")
INC = ["-I" + os.path.join(ROOT, "tools", "hipemu"), "-I" + os.path.join(ROOT, "mash_amd", "csrc")]
CASES = ["small", "star", "between", "ties", "zero", "band", "lengths", "padding", "overflow"]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("emu") / "cluster_nearest_emu")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-DMG_HIP_EMU", "-DHIPEMU_FIBERS", *INC, SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize("case", CASES)
def test_nearest_kernels_on_the_cpu(emu, case):
    r = subprocess.run([emu, case], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "all cases agree" in r.stdout and "FAIL" not in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_nearest_kernels_on_the_cpu_random_jobs(emu):
    """`cluster_nearest_emu fuzz <seed> <cases>`: seed 20261020, 100 jobs: 2 .. 20 000 rows, one to three appends over one list
    (lists of up to 6 000 distinct pairs named either way round, or row blocks of a flat triangle), mask densities from 1 to 1e-3,
    edges inside 1 .. 40 families, counts in quarters of 64 and 32 and 0/0 (ties across denominators are common), every third job
    with a first capacity of 1 .. 5 000 edges"""
    r = subprocess.run([emu, "fuzz", "20261020", "100"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "all cases agree" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    moved = [ln for ln in r.stdout.splitlines() if ln.startswith("ok") and " 0 members not under their first" not in ln]
    later = [ln for ln in r.stdout.splitlines() if ln.startswith("ok") and ", 0 under a later one" not in ln]
    assert len(moved) >= 20 and len(later) >= 20                     # the jobs do tell the two rules apart


def test_nearest_kernels_under_thread_sanitizer(tmp_path):
    exe = str(tmp_path / "cluster_nearest_emu_tsan")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=thread", "-DMG_HIP_EMU", "-pthread", *INC, SRC, "-o", exe], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("no ThreadSanitizer runtime here: " + r.stderr[-200:])
    r = subprocess.run([exe, "small"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "all cases agree" in r.stdout and "ThreadSanitizer" not in r.stderr, r.stdout[-2000:] + r.stderr[:3000]
