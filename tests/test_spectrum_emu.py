"""The kernels of `mash triangle -H` / `mash dist -H`, unchanged, through their launchers on the CPU (tools/hipemu: work-items as
fibers): sp_marked_kernel, sp_all_kernel and sp_list_kernel of mash_amd/csrc/spectrum.hip, each in the combining variant and in the
plain one, against a sequential C++ restatement: pair counts that are not a multiple of 64, the first words of a flat triangle, a
single set bit in a word's last lane, pair spaces that exclude set bits, two and five pieces over one set of bins, the list form with
both binnings, s = 64, 1000, 16 383, 16 384 and 20 000 (LDS and global homes), every entry in one bin (s/s, 0/s without masks, one key
of the table), denominators 63, 64, 32 and 0 mixed, a table started at 4 slots until it has regrown, and random jobs with a fixed
seed.  Guard words stand behind every array.  The emulator runs workgroups one after another: the races between workgroups on one
bin are exercised on the device only (tests/test_spectrum_gpu.py).  One small case also runs with work-items as OS threads under
ThreadSanitizer."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emu", "spectrum_emu_main.cpp")
INC = ["-I" + os.path.join(ROOT, "tools", "hipemu"), "-I" + os.path.join(ROOT, "mash_amd", "csrc")]
CASES = ["small", "lengths", "words", "space", "pieces", "lists", "sizes", "hot", "denoms", "regrow"]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("emu") / "spectrum_emu")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-DMG_HIP_EMU", "-DHIPEMU_FIBERS", *INC, SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize("case", CASES)
def test_spectrum_kernels_on_the_cpu(emu, case):
    r = subprocess.run([emu, case], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "all cases agree" in r.stdout and "FAIL" not in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_spectrum_kernels_on_the_cpu_random_jobs(emu):
    """`spectrum_emu fuzz <seed> <cases>`: seed 20261021, 100 jobs: s of 64, 200, 1000 or 20 000; one to three pieces of a flat
    triangle of up to 251 rows, marked (densities 1 to 1/8, some with a pair space) or whole, or a list of up to 220 rows with both
    binnings; counts hot in 0/d and in one middle key or spread; a table started at 4, 64 or 1024 slots; both variants"""
    r = subprocess.run([emu, "fuzz", "20261021", "100"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "all cases agree" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    ok = [ln for ln in r.stdout.splitlines() if ln.startswith("ok")]
    others = [ln for ln in ok if int(re.search(r", (\d+) with another denominator", ln).group(1)) > 0]
    regrown = [ln for ln in ok if int(re.search(r", (\d+) regrows", ln).group(1)) > 0]
    assert len(ok) == 100 and len(others) >= 20 and len(regrown) >= 20, (len(ok), len(others), len(regrown))


def test_spectrum_kernels_under_thread_sanitizer(tmp_path):
    exe = str(tmp_path / "spectrum_emu_tsan")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=thread", "-DMG_HIP_EMU", "-pthread", *INC, SRC, "-o", exe], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("no ThreadSanitizer runtime here: " + r.stderr[-200:])
    r = subprocess.run([exe, "small"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "all cases agree" in r.stdout and "ThreadSanitizer" not in r.stderr, r.stdout[-2000:] + r.stderr[:3000]
