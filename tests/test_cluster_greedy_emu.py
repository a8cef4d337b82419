"""mash_amd/csrc/cluster_greedy.hip, unchanged, through its launchers (cg_append_kernel in list mode and in flat triangle mode,
the rounds of cg_round_edges_kernel and cg_round_rows_kernel in batches, cg_rep_init_kernel and cg_assign_kernel) on the CPU
(tools/hipemu: work-items as fibers) against the sequential walk over the same edges: a path in index order (the deepest chain:
a round decides two rows) and over shuffled rows, band graphs, stars around row 0 and around a middle row (which must NOT
collect the rows below it), a clique of 1 500 rows in flat order (1 124 250 pairs: not a multiple of 64), mask words of every
density from 0 to 64 bits, lists whose length is not a multiple of 64, row blocks of one triangle over one list and one state
array, lists that overflow and are regrown (a first capacity of 1 edge, inside a word, one short, exactly enough), tables of 0
and 1 rows, and random jobs with a fixed seed.  Checked: rep, the number of clusters, what every append leaves in the list, the
cursor and the overflow flag, the words behind every array, that rounds queued behind the fixpoint do nothing and that the
number of rounds never exceeds n.
The emulator runs workgroups one after another: the races between workgroups are exercised on the device only
(tests/test_cluster_greedy_gpu.py).  One small case also runs with work-items as OS threads under ThreadSanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emu", "cluster_greedy_emu_main.cpp")
INC = ["-I" + os.path.join(ROOT, "tools", "hipemu"), "-I" + os.path.join(ROOT, "mash_amd", "csrc")]
CASES = ["small", "path", "band", "star", "clique", "density", "blocks", "overflow"]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("emu") / "cluster_greedy_emu")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-DMG_HIP_EMU", "-DHIPEMU_FIBERS", *INC, SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize("case", CASES)
def test_greedy_kernels_on_the_cpu(emu, case):
    r = subprocess.run([emu, case], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "all cases agree" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_greedy_kernels_on_the_cpu_random_jobs(emu):
    """`cluster_greedy_emu fuzz <seed> <cases>`: seed 20261017, 120 jobs: 2 .. 20 000 rows, one to three appends over one list
    (lists of up to 60 000 pairs named either way round, or row blocks of a flat triangle), mask densities from 1 to 1e-4, edges
    inside 1 .. 40 families, every third job with a first capacity of 1 .. 5 000 edges"""
    r = subprocess.run([emu, "fuzz", "20261017", "120"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "all cases agree" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_greedy_kernels_under_thread_sanitizer(tmp_path):
    exe = str(tmp_path / "cluster_greedy_emu_tsan")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=thread", "-DMG_HIP_EMU", "-pthread", *INC, SRC, "-o", exe], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("no ThreadSanitizer runtime here: " + r.stderr[-200:])
    r = subprocess.run([exe, "small"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "all cases agree" in r.stdout and "ThreadSanitizer" not in r.stderr, r.stdout[-2000:] + r.stderr[:3000]
