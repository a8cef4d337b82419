"""mash_amd/csrc/cluster.hip, unchanged, through its launchers (cl_init_kernel, cl_union_kernel in list mode and in flat triangle
mode, cl_label_kernel) on the CPU (tools/hipemu: work-items as fibers) against a sequential union-find over the same edges:
a path listed in descending and ascending order, stars around row 0 and around a middle row, a clique of 2 000 rows in flat
order (1 999 000 pairs: not a multiple of 64), two components of 3 000 interleaved rows joined by the last edge, mask words of
every density from 0 to 64 bits, lists and triangles whose pair count is not a multiple of 64, row blocks of one triangle over
one persistent parent array, tables of 0 and 1 rows, and random jobs with a fixed seed.  Labels, the number of clusters, the
invariant parent[x] <= x after every launch and the words behind the arrays are checked.
The emulator runs workgroups one after another: the races between workgroups are exercised on the device only
(tests/test_cluster_gpu.py).  One small case also runs with work-items as OS threads under ThreadSanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emu", "cluster_emu_main.cpp")
INC = ["-I" + os.path.join(ROOT, "tools", "hipemu"), "-I" + os.path.join(ROOT, "mash_amd", "csrc")]
CASES = ["small", "path", "star", "clique", "bridge", "density", "ragged", "blocks"]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("emu") / "cluster_emu")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-DMG_HIP_EMU", "-DHIPEMU_FIBERS", *INC, SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize("case", CASES)
def test_cluster_kernels_on_the_cpu(emu, case):
    r = subprocess.run([emu, case], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "all cases agree" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_cluster_kernels_on_the_cpu_random_jobs(emu):
    """`cluster_emu fuzz <seed> <cases>`: seed 20261017, 150 jobs: 2 .. 20 000 rows, one to three launches over one parent array
    (lists of up to 60 000 pairs, or row blocks of a flat triangle), mask densities from 1 to 1e-4, edges inside 1 .. 40 families"""
    r = subprocess.run([emu, "fuzz", "20261017", "150"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "all cases agree" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_cluster_kernels_under_thread_sanitizer(tmp_path):
    exe = str(tmp_path / "cluster_emu_tsan")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=thread", "-DMG_HIP_EMU", "-pthread", *INC, SRC, "-o", exe], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("no ThreadSanitizer runtime here: " + r.stderr[-200:])
    r = subprocess.run([exe, "small"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "all cases agree" in r.stdout and "ThreadSanitizer" not in r.stderr, r.stdout[-2000:] + r.stderr[:3000]
