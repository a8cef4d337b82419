"""The inverted-index engine of mash_amd/csrc/compare_sparse.hip -- sp_locate, sp_discover (count-only and listing, with and
without classes of copies), the six merge forms (one lane per candidate, the whole row in LDS, the row a window at a time,
several rows per item at 32 / 43 / 64 units), sp_scatter, sp_class_pairs, sp_fill_short, all through the library's launchers
(their two device scans replaced by std::partial_sum) -- run on the CPU (tools/hipemu: work-items as fibers) on index arrays
made by a std::stable_sort.  EVERY pair of the output is compared with the loop of compareSketches (CommandDistance.cpp:347-385),
the six forms' results must be byte-equal, a form its launcher declines is reported, and discovery is checked on its own
(counters, the candidate set, segment order, a list too small).  Tables built for the kernels' edges: tests/emu/sparse_emu_main.cpp,
whose header also lists the mutations of the kernel file each case catches."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emu", "sparse_emu_main.cpp")
INC = ["-I" + os.path.join(ROOT, "tools", "hipemu"), "-I" + os.path.join(ROOT, "mash_amd", "csrc")]
CASES = ["sizes", "ring", "chunks", "pack", "windows", "copies", "rect", "discover"]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("emu") / "sparse_emu")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-DMG_HIP_EMU", "-DHIPEMU_FIBERS", *INC, SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize("case", CASES)
def test_sparse_kernels_on_the_cpu(emu, case):
    r = subprocess.run([emu, case], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "all cases agree" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_sparse_kernels_on_the_cpu_random_tables(emu):
    """tables of random shape (2 .. 300 rows, s 1 .. 150 and now and then above 2052; pools, trees, pools with copies, ragged
    rows; triangle with row ranges, visiting orders and permuted indexes, and rect with query sketch sizes of their own; the
    lanes form and one other form per table): `sparse_emu fuzz <seed> <cases>`; 150 cases of five other seeds ran clean when
    this was written"""
    r = subprocess.run([emu, "fuzz", "20261020", "8"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "all cases agree" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
