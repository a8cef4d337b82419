"""K3 of the index build (index_build.hip: the tile partition) alone, on the CPU (tools/hipemu), with both of its bodies -- the
ranks taken in registers and the LSD sort in LDS (MASHGPU_IX_PARTITION=rank|lsd).  pk and the slot image must be equal word for
word between the bodies and to a std::stable_sort statement: by bucket, then row, then position.
  table      n = 1 100 (two full blocks of rows and a ragged third), s = 96 in rows of stride 104; full, short and empty rows, one
             value held by 300 rows; maps: identity, reversal, a seeded random permutation; several windows, and one window, where
             a full block's tile is 49 000 entries taken in 14 pieces;
  long       rows of 100, 700 and 4 100 entries in one window (across a step of 64, a wave's share, a piece), a long row in one
             bucket, a window with no entries, a last block of one row;
  runs       a tile whose 4 608 entries all fall into one bucket; a run of one bucket across the waves' shares and the piece;
  bw1, bw2, bw512   1, 2 and 512 buckets per window;
  one_tile   one tile, which is also what runs under ThreadSanitizer (work-items as OS threads: a wave operation missing between
             the peers' read of a counter and its owner's write is a reported race)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emu", "index_partition_emu_main.cpp")
INC = ["-I" + os.path.join(ROOT, "tools", "hipemu"), "-I" + os.path.join(ROOT, "mash_amd", "csrc")]

TABLE = [("table", m, w) for m in ("identity", "reversal", "random") for w in ("one", "several")]
HAND = [("long",), ("runs",), ("bw1",), ("bw2",), ("bw512",), ("one_tile",)]
CASES = TABLE + HAND


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """every case as a process of its own, side by side (a case is one thread of context switches)"""
    from concurrent.futures import ThreadPoolExecutor
    exe = str(tmp_path_factory.mktemp("emu") / "index_partition_emu")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-DMG_HIP_EMU", "-DHIPEMU_FIBERS", *INC, SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(case):
        return subprocess.run([exe, *case], capture_output=True, text=True, timeout=900)
    with ThreadPoolExecutor(max_workers=max(1, min(8, (os.cpu_count() or 2) // 2))) as ex:
        return dict(zip(CASES, ex.map(run, CASES)))


@pytest.mark.parametrize("rowmap,windows", [c[1:] for c in TABLE])
def test_both_bodies_equal_the_stable_sort(runs, rowmap, windows):
    r = runs[("table", rowmap, windows)]
    assert r.returncode == 0 and ": equal" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.parametrize("case", [c[0] for c in HAND])
def test_both_bodies_on_hand_made_geometries(runs, case):
    r = runs[(case,)]
    assert r.returncode == 0 and ": equal" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_one_tile_under_thread_sanitizer(tmp_path):
    exe = str(tmp_path / "index_partition_emu_tsan")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=thread", "-DMG_HIP_EMU", "-pthread", *INC, SRC, "-o", exe], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("no ThreadSanitizer runtime here: " + r.stderr[-200:])
    r = subprocess.run([exe, "one_tile"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and ": equal" in r.stdout and "ThreadSanitizer" not in r.stderr, r.stdout[-2000:] + r.stderr[:3000]
