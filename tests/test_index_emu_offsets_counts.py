"""The window offsets and the blocks' bucket counts from one read of the table (index_build.h: index_offsets_counts): the kernels
run on the CPU (tools/hipemu).  lb and cnt of the fused kernel must equal those of K0 + K1 word for word, and the whole build
behind them (stage bits 8 | 16) the build that runs K0 + K1 itself, in every array.  n = 1 100 (two full blocks of rows and a
ragged third), s = 96 in rows of stride 104; full, short and empty rows, one value held by 300 rows; maps: identity, reversal,
a seeded random permutation; one window and several.  The carry case: 512 equal rows of s = 160 whose values fall into two
neighbouring buckets of a hand-made geometry, 66 560 entries for a 16-bit counter -- flags[IXF_DEGENERATE] must be raised (the
general sort, where such a table goes, is not run here).  The route rule: 81 888 buckets (2 Bp + 64 bytes = 160 KB) take the
fused kernel, 81 889 the tiles' K0 + K1."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emu", "index_offsets_counts_emu_main.cpp")
INC = ["-I" + os.path.join(ROOT, "tools", "hipemu"), "-I" + os.path.join(ROOT, "mash_amd", "csrc")]

EQUAL = [(m, w) for m in ("identity", "reversal", "random") for w in ("one", "several")]
CASES = EQUAL + [("carry",), ("route",)]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """every case as a process of its own, side by side (a case is one thread of context switches)"""
    from concurrent.futures import ThreadPoolExecutor
    exe = str(tmp_path_factory.mktemp("emu") / "index_offsets_counts_emu")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-DMG_HIP_EMU", "-DHIPEMU_FIBERS", *INC, SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(case):
        return subprocess.run([exe, *case], capture_output=True, text=True, timeout=900)
    with ThreadPoolExecutor(max_workers=max(1, min(8, (os.cpu_count() or 2) // 2))) as ex:
        return dict(zip(CASES, ex.map(run, CASES)))


@pytest.mark.parametrize("rowmap,windows", EQUAL)
def test_fused_offsets_and_counts_equal_k0_k1(runs, rowmap, windows):
    r = runs[(rowmap, windows)]
    assert r.returncode == 0 and ": equal" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_counter_overflow_raises_the_flag(runs):
    r = runs[("carry",)]
    assert r.returncode == 0 and ": caught" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_route_rule_at_the_lds_limit(runs):
    r = runs[("route",)]
    assert r.returncode == 0 and ": as stated" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
