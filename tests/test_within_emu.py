"""The kernels of mash_amd/csrc/within.hip -- within_last_kernel, within_j_kernel and both forms of within_count_kernel (a
block of the matrix; the list of a threshold's survivors) -- run unchanged on the CPU (tools/hipemu: work-items as fibers)
against a literal transcription of the reference's serial walk (containSketches, CommandContain.cpp:231-263): sketch sizes 1, 5,
64, 65, 1000 and 5000 on tables of 1 to 72 rows, tables of different sketch sizes either way round, rows of 0, 1 and fewer than
s hashes, a real hash equal to the padding value, values below 2^32, one reference and one query, sub-ranges of the queries
(an empty one too), j_min on both sides of the rows' hash counts, and disjoint value ranges in both orders."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emu", "within_emu_main.cpp")
INC = ["-I" + os.path.join(ROOT, "tools", "hipemu"), "-I" + os.path.join(ROOT, "mash_amd", "csrc")]
CASES = ["sizes", "mixed", "short", "pad", "hash32", "single", "ranges", "jmin", "disjoint"]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("emu") / "within_emu")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-DMG_HIP_EMU", "-DHIPEMU_FIBERS", *INC, SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize("case", CASES)
def test_within_kernels_on_the_cpu(emu, case):
    r = subprocess.run([emu, case], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "all cases agree" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_within_kernels_on_the_cpu_random_jobs(emu):
    """`within_emu fuzz <seed> <cases>`: seed 20261021, 150 jobs of random shape (1 .. 20 rows a side, sketch sizes of 1 .. 700
    chosen per side, full and ragged rows, 64- and 32-bit values, any j_min); all three ways the walk ends must occur"""
    r = subprocess.run([emu, "fuzz", "20261021", "150"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "all cases agree" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
