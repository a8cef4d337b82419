"""The launchers that extend an earlier clustering -- mash_amd/csrc/cluster.hip (launch_cluster_seed, launch_cluster_union with a
base per side, launch_cluster_label) and mash_amd/csrc/cluster_greedy.hip (launch_greedy_append with a base per side,
launch_greedy_seed, the rounds, launch_greedy_assign for the new rows only) -- unchanged, on the CPU (tools/hipemu: work-items as
fibers) against a sequential statement of both definitions: the seed then rect ballots in flat mode with ncols 1, 63 and 65 and
pair counts that are no multiple of 64, list mode, rect blocks then tri blocks over one parent and one edge list, a new row
bridging two old clusters, new rows beside old clusters only through other new rows, new rows without edges, n = 0, m = 0,
m = 1, mask words of every density from 0 to 64 bits; greedy: a new row beside an old MEMBER only (it must become a
representative), a new row beside an old REP (its member), a chain of new rows in index order, the list overflowing once and
regrown; and random jobs with a fixed seed.  Checked after every launch: parent[x] <= x and the guard words behind the arrays;
at the end: label, rep of the new rows, both cluster counts, what every append left in the list, that the old rows' states never
change.
The emulator runs workgroups one after another: the races between workgroups are exercised on the device only
(tests/test_cluster_extend_gpu.py).  One small case also runs with work-items as OS threads under ThreadSanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emu", "cluster_extend_emu_main.cpp")
INC = ["-I" + os.path.join(ROOT, "tools", "hipemu"), "-I" + os.path.join(ROOT, "mash_amd", "csrc")]
CASES = ["small", "flat", "list", "blocks", "bridge", "chain", "density", "greedy", "overflow"]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("emu") / "cluster_extend_emu")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-DMG_HIP_EMU", "-DHIPEMU_FIBERS", *INC, SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize("case", CASES)
def test_extend_kernels_on_the_cpu(emu, case):
    r = subprocess.run([emu, case], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "all cases agree" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_extend_kernels_on_the_cpu_random_jobs(emu):
    """`cluster_extend_emu fuzz <seed> <cases>`: seed 20261020, 150 jobs: 0 .. 8 000 old rows under a random earlier partition (every
    fourth job: all representatives, the greedy seed NULL), 0 .. 3 000 new rows, rect and tri jobs as lists (tri pairs named either
    way round) or as row blocks of the flat layouts, mask densities from 1 to 1e-4, edges inside 1 .. 40 families, every third job
    with a first capacity of 1 .. 5 000 edges"""
    r = subprocess.run([emu, "fuzz", "20261020", "150"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "all cases agree" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_extend_kernels_under_thread_sanitizer(tmp_path):
    exe = str(tmp_path / "cluster_extend_emu_tsan")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=thread", "-DMG_HIP_EMU", "-pthread", *INC, SRC, "-o", exe], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("no ThreadSanitizer runtime here: " + r.stderr[-200:])
    r = subprocess.run([exe, "small"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "all cases agree" in r.stdout and "ThreadSanitizer" not in r.stderr, r.stdout[-2000:] + r.stderr[:3000]
