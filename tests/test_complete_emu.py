"""mash_amd/csrc/cluster_complete.hip, unchanged, through its launchers (the keys and the open-addressing lookup of
launch_complete_begin; the rounds K1 .. K5 as launch_complete_rounds queues them, in batches that double) behind cluster_forest.hip's
append and in front of cluster.hip's labels, on the CPU (tools/hipemu: work-items as fibers) against a sequential walk of the
definition written in the test program: a clique of equal fractions (n - 1 merging rounds, one cluster), the same with one edge
missing (two overlapping cliques: the tie rule decides who wins) and with that row's edges better, a path (pairs, never triples),
two cliques joined by their best and by their worst edge, a round in which BOTH ends of a surviving link merge (three lookups) with
one of the four links absent and with all four there, a dropped weight that decides the next merge, equal fractions under several
denominators and denominators of 2^21 - 1, a list regrown from a capacity of 1, several appends over one list (row blocks, lists
with pairs no bit marks), every link hashed to slot 0 and to the table's last slot (the probe wraps round its end), a fixpoint on,
before and behind a batch boundary, tables of 0, 1 and 2 rows, and random jobs with a fixed seed.
Checked: the labels, the number of clusters and of merges, that every cluster is a clique, what the lookup holds, the words behind
every array, live[] and merged[] of every round, that rounds queued behind the fixpoint change nothing, and the rows' round state
as the last round left it.
The emulator runs workgroups one after another: the races between workgroups are exercised on the device only
(tests/test_complete_gpu.py).  One small case also runs with work-items as OS threads under ThreadSanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emu", "complete_emu_main.cpp")
INC = ["-I" + os.path.join(ROOT, "tools", "hipemu"), "-I" + os.path.join(ROOT, "mash_amd", "csrc")]
CASES = ["small", "clique", "path", "joined", "both", "denoms", "lists", "hash", "batches"]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("emu") / "complete_emu")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-DMG_HIP_EMU", "-DHIPEMU_FIBERS", *INC, SRC, "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize("case", CASES)
def test_complete_kernels_on_the_cpu(emu, case):
    r = subprocess.run([emu, case], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "all cases agree" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_complete_kernels_on_the_cpu_random_jobs(emu):
    """`complete_emu fuzz <seed> <cases>`: seed 20261021, 40 jobs: 2 .. 3 000 rows in families of 2 .. 41 rows that are cliques
    with none to 45 % of their edges missing, n / 4 edges between families, 1 .. 16 fraction values under three denominators, one to
    three lists (some with pairs no bit marks) or row blocks of a flat triangle, every third job with a first capacity of 1 .. 5 000
    edges, first batches of 1 .. 8 rounds, every fourth job with sixteen home slots in the lookup"""
    r = subprocess.run([emu, "fuzz", "20261021", "40"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "all cases agree" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_complete_kernels_under_thread_sanitizer(tmp_path):
    exe = str(tmp_path / "complete_emu_tsan")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=thread", "-DMG_HIP_EMU", "-pthread", *INC, SRC, "-o", exe], capture_output=True, text=True,
                       timeout=600)
    if r.returncode != 0:
        pytest.skip("no ThreadSanitizer runtime here: " + r.stderr[-200:])
    r = subprocess.run([exe, "small"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "all cases agree" in r.stdout and "ThreadSanitizer" not in r.stderr, r.stdout[-2000:] + r.stderr[:3000]
