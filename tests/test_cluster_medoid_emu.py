"""The kernels of `mash cluster -M`, unchanged, through their launchers on the CPU (tools/hipemu: work-items as fibers):
cm_union_kernel of mash_amd/csrc/cluster_medoid.hip in both variants (a row's weights combined in the wave; two atomics per edge),
cl_label_kernel of cluster.hip and launch_medoid_pick (cm_best_kernel, cm_pick_kernel, cm_medoid_kernel), against a sequential C++
restatement: pair counts that are not a multiple of 64, the first words of a flat triangle (one word spans rows 1 .. 11), words
that span exactly two rows, a word with a single set bit in its last lane, list jobs with rows unsorted and the same row in
lanes far apart (more distinct rows in a word than the wave combines included), pair spaces that exclude some set bits, two,
three and five row blocks over one score[], 0/0 and 0/d edges, denominators 63, 64 and 32 mixed (21/63: a weight that is no
multiple of 2^-32), a clique, a star whose centre is the LAST row, a path, two clusters interleaved in index order, the band
whose scores have a closed form, exact ties (the smallest row wins), tables of 0 and 1 rows, and random jobs with a fixed seed.
The emulator runs workgroups one after another: the races between workgroups on score[], best[] and pick[] are exercised on
the device only (tests/test_cluster_medoid_gpu.py).  One small case also runs with work-items as OS threads under ThreadSanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emu", "cluster_medoid_emu_main.cpp")
INC = ["-I" + os.path.join(ROOT, "tools", "hipemu"), "-I" + os.path.join(ROOT, "mash_amd", "csrc")]
CASES = ["small", "lengths", "words", "lists", "space", "blocks", "weights", "shapes", "ties"]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("emu") / "cluster_medoid_emu")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-DMG_HIP_EMU", "-DHIPEMU_FIBERS", *INC, SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize("case", CASES)
def test_medoid_kernels_on_the_cpu(emu, case):
    r = subprocess.run([emu, case], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "all cases agree" in r.stdout and "FAIL" not in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_medoid_kernels_on_the_cpu_random_jobs(emu):
    """`cluster_medoid_emu fuzz <seed> <cases>`: seed 20261020, 100 jobs: 2 .. 20 000 rows, one to three launches over one score[]
    (lists of up to 6 000 distinct pairs named either way round, or row blocks of a flat triangle), mask densities from 1 to 1e-3,
    edges inside 1 .. 40 families, counts in quarters of 64 and 32, thirds of 63 and 0/0 (ties are common), both variants"""
    r = subprocess.run([emu, "fuzz", "20261020", "100"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "all cases agree" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    ok = [ln for ln in r.stdout.splitlines() if ln.startswith("ok")]
    moved = [ln for ln in ok if ", 0 with a medoid that is not their first member" not in ln]
    ties = [ln for ln in ok if ", 0 with a tie for the top score" not in ln]
    assert len(ok) == 100 and len(moved) >= 20 and len(ties) >= 20       # the jobs do tell the medoid from the first member


def test_medoid_kernels_under_thread_sanitizer(tmp_path):
    exe = str(tmp_path / "cluster_medoid_emu_tsan")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=thread", "-DMG_HIP_EMU", "-pthread", *INC, SRC, "-o", exe], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("no ThreadSanitizer runtime here: " + r.stderr[-200:])
    r = subprocess.run([exe, "small"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "all cases agree" in r.stdout and "ThreadSanitizer" not in r.stderr, r.stdout[-2000:] + r.stderr[:3000]
