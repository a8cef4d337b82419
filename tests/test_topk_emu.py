"""The two selection kernels of mash_amd/csrc/topk.hip, through launch_topk_select -- topk_select_kernel (rows of more than
64 pairs: the streamed row, ballots, the bitonic prune, the bound) and topk_select_short_kernel (a wave per row of up to 64
pairs: the lists of 0, 1, 2, 5, 63 and 64 pairs of `short`, the short lists of `bits`, and the fuzz jobs' short lists and
matrices of 64 columns and fewer) -- run on the CPU (tools/hipemu: work-items as fibers) against a std::stable_sort statement of the definition of `mash dist -N`,
with the fractions compared in 128-bit integers: all fractions equal, ties that straddle every tested k (1, 3, 10, 100, 1024),
fewer eligible pairs than k, sparse eligibility masks at every bit offset, rows ten LDS buffers long (ascending, so that every
chunk beats the bound; descending; random), and the neighbours no float32 or 32-bit quotient separates, denominators up to
2^32 - 1; matrix rows and candidate lists."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emu", "topk_emu_main.cpp")
INC = ["-I" + os.path.join(ROOT, "tools", "hipemu"), "-I" + os.path.join(ROOT, "mash_amd", "csrc")]
CASES = ["ties", "cut", "short", "bits", "long", "farey"]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("emu") / "topk_emu")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-DMG_HIP_EMU", "-DHIPEMU_FIBERS", *INC, SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize("case", CASES)
def test_topk_selection_on_the_cpu(emu, case):
    r = subprocess.run([emu, case], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "all cases agree" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_topk_selection_on_the_cpu_random_jobs(emu):
    """`topk_emu fuzz <seed> <cases>`: seed 20261017, 120 jobs of random shape (matrix rows of 1 .. 5000 pairs or lists of
    0 .. 5000, s of 1 .. 100 000, ragged denominators, any share of zero numerators, any mask density, k of 1 .. 1024)"""
    r = subprocess.run([emu, "fuzz", "20261017", "120"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "all cases agree" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
