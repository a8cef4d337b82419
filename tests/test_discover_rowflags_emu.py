"""The rows' flags that let discovery leave a row without scanning it (SparseArgs::row_any; index_build.hip: K5 sets them,
compare_dense.hip: the encode writes them again for the rows of dense groups), with the kernels run on the CPU (tools/hipemu).
A table of 589 rows of s = 100 (a ragged second block of 77 rows; pieces of 32 positions, the last one ragged): unrelated rows,
an empty row, four clades of 16 - 40 near-copies kept as dense groups, two of them with values planted across them, two rows
outside every group that share values with clade rows and with each other, a row of 45 entries whose only non-empty run is
its last entry and a row whose only one is its first.  Behind K5, and again behind dn_encode_kernel<1> and <8>, every row's
flag must equal what a plain loop over the images says; the rows of a clade on its own are flagged by K5 and cleared by the
encode; rows outside the groups keep K5's flag; the verify mode's kernel agrees, and counts a flag turned either way.
Once more under AddressSanitizer and UndefinedBehaviorSanitizer (the emulator's thread back end: a stand-alone program)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emu", "discover_rowflags_emu_main.cpp")
INC = ["-I" + os.path.join(ROOT, "tools", "hipemu"), "-I" + os.path.join(ROOT, "mash_amd", "csrc")]


def _build_and_run(tmp_path, name, flags, *args):
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-DMG_HIP_EMU", *flags, *INC, SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=900)


@pytest.mark.parametrize("seed", ["20261021", "7"])
def test_flags_equal_a_scan_of_the_images(tmp_path, seed):
    r = _build_and_run(tmp_path, "discover_rowflags_emu", ["-DHIPEMU_FIBERS"], seed)
    assert r.returncode == 0 and ": as the images say" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_flags_under_asan_and_ubsan(tmp_path):
    r = _build_and_run(tmp_path, "discover_rowflags_emu_san",
                       ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread"])
    assert r.returncode == 0 and ": as the images say" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
