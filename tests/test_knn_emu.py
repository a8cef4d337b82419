"""The mirror of mash_amd/csrc/knn.hip (degree pass, multi-workgroup scan, scatter) and the keyed selection of topk.hip
(launch_topk_select_keyed: the wave kernel and the long kernel) run on the CPU (tools/hipemu: work-items as fibers) against a
std::stable_sort statement of the definition of `mash triangle -N`, with the fractions compared in 128-bit integers: all
fractions equal (pure neighbour order across the diagonal), ties that straddle every tested k (1, 3, 10, 100, 1024), a first
row with a mirrored half only and a last row with an own half only, rows without an eligible neighbour, degrees 0, 1, 63, 64,
65, 1024, 1025 and 2500, eligibility bits at every offset of a ballot word.  Every job runs twice, its list entries in
reference order and shuffled: the order inside a mirrored segment is unspecified and the answer must not depend on it."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emu", "knn_emu_main.cpp")
INC = ["-I" + os.path.join(ROOT, "tools", "hipemu"), "-I" + os.path.join(ROOT, "mash_amd", "csrc")]
CASES = ["equal", "straddle", "ends", "degrees", "bits"]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("emu") / "knn_emu")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-DMG_HIP_EMU", "-DHIPEMU_FIBERS", *INC, SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize("case", CASES)
def test_knn_mirror_and_keyed_selection_on_the_cpu(emu, case):
    r = subprocess.run([emu, case], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "all cases agree" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_knn_mirror_and_keyed_selection_on_the_cpu_random_jobs(emu):
    """`knn_emu fuzz <seed> <cases>`: seed 20261019, 24 jobs of random shape (1 .. 2500 rows, any share of the pairs listed, any
    share of those eligible, s of 1 .. 100 000, ragged denominators, any share of zero numerators, k of 1 .. 1024)"""
    r = subprocess.run([emu, "fuzz", "20261019", "24"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "all cases agree" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
