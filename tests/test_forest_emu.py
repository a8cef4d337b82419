"""mash_amd/csrc/cluster_forest.hip, unchanged, through its launchers (cf_append_kernel in list mode and in flat triangle mode; the
Boruvka rounds, the labels, the padding, the bitonic sort and the denominator flags as launch_forest_rounds queues them) on the CPU
(tools/hipemu: work-items as fibers) against Kruskal over the same edges under a comparator of the test program's own: a path in
index order (with mixed weights and with one weight) and over shuffled rows, a clique whose fractions are all equal (the forest must
be the star around row 0) and the same with one row's edges better, a star around a middle row, a disconnected graph, equal
fractions under several denominators (1/2, 2/4, 32/64) and denominators of 2^21 - 1, mask words of every density from 0 to 64 bits,
lists whose length is no multiple of 64, row blocks of one triangle over one list, lists that overflow and are regrown (a first
capacity of 1 edge, inside a word, one short, exactly enough), tables of 0, 1 and 2 rows, and random jobs with a fixed seed.
Checked: the records and their order, label, the counts, what every append leaves in the list, the cursor and the overflow flag,
the words behind every array, the padding, the denominator flags, that rounds queued behind the fixpoint choose nothing and leave
comp / best_key / best_rc as the fixpoint left them, and rounds <= floor(log2 n) + 1.
The emulator runs workgroups one after another: the races between workgroups are exercised on the device only
(tests/test_forest_gpu.py).  One small case also runs with work-items as OS threads under ThreadSanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emu", "forest_emu_main.cpp")
INC = ["-I" + os.path.join(ROOT, "tools", "hipemu"), "-I" + os.path.join(ROOT, "mash_amd", "csrc")]
CASES = ["small", "path", "clique", "star", "parts", "denoms", "density", "blocks", "overflow"]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("emu") / "forest_emu")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-DMG_HIP_EMU", "-DHIPEMU_FIBERS", *INC, SRC, "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize("case", CASES)
def test_forest_kernels_on_the_cpu(emu, case):
    r = subprocess.run([emu, case], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "all cases agree" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_forest_kernels_on_the_cpu_random_jobs(emu):
    """`forest_emu fuzz <seed> <cases>`: seed 20261019, 60 jobs: 2 .. 6 000 rows, one to three appends over one list (lists of up to
    30 000 pairs named either way round, or row blocks of a flat triangle), mask densities from 1 to 1e-3, edges inside 1 .. 20
    families, 1 .. 16 fraction values under three denominators, every third job with a first capacity of 1 .. 5 000 edges"""
    r = subprocess.run([emu, "fuzz", "20261019", "60"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "all cases agree" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_forest_kernels_under_thread_sanitizer(tmp_path):
    exe = str(tmp_path / "forest_emu_tsan")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=thread", "-DMG_HIP_EMU", "-pthread", *INC, SRC, "-o", exe], capture_output=True, text=True,
                       timeout=600)
    if r.returncode != 0:
        pytest.skip("no ThreadSanitizer runtime here: " + r.stderr[-200:])
    r = subprocess.run([exe, "small"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "all cases agree" in r.stdout and "ThreadSanitizer" not in r.stderr, r.stdout[-2000:] + r.stderr[:3000]
