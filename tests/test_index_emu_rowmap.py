"""The index build reads the table in place through a row map (index_build.h: index_build_mapped, index_window_offsets): the
kernels run on the CPU (tools/hipemu) on a table T with a map pi, and on the materialised copy T o pi without one; every
array of the two builds must be equal word for word -- values, rows, group starts and ends, both images, statistics and
flags, the window offsets, the partition's scratch -- and K0 queued ahead of the build (counts in the table's order) must
leave the same window offsets.  n = 1 100 (two full blocks of rows and a ragged third), s = 96 in rows of stride 104; full,
short and empty rows, one value held by 300 rows; maps: identity, reversal, a seeded random permutation; one window and several."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emu", "index_rowmap_emu_main.cpp")
INC = ["-I" + os.path.join(ROOT, "tools", "hipemu"), "-I" + os.path.join(ROOT, "mash_amd", "csrc")]

CASES = [(m, w) for m in ("identity", "reversal", "random") for w in ("one", "several")]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """every case as a process of its own, side by side (a case is one thread of context switches)"""
    from concurrent.futures import ThreadPoolExecutor
    exe = str(tmp_path_factory.mktemp("emu") / "index_rowmap_emu")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-DMG_HIP_EMU", "-DHIPEMU_FIBERS", *INC, SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(case):
        return subprocess.run([exe, *case], capture_output=True, text=True, timeout=900)
    with ThreadPoolExecutor(max_workers=max(1, min(6, (os.cpu_count() or 2) // 2))) as ex:
        return dict(zip(CASES, ex.map(run, CASES)))


@pytest.mark.parametrize("rowmap,windows", CASES)
def test_mapped_build_equals_the_build_on_the_copy(runs, rowmap, windows):
    r = runs[(rowmap, windows)]
    assert r.returncode == 0 and ": equal" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
