"""The kernels of `mash cluster -D`, unchanged, through their launchers on the CPU (tools/hipemu: work-items as fibers):
cf_append_kernel of mash_amd/csrc/cluster_forest.hip and launch_density of mash_amd/csrc/cluster_density.hip (the degree pass in
both forms, the core union, the labels, the border's key and pick, the relabelling), against a sequential C++ restatement that uses
forest_before: a bridge row between two cliques, nearer the later one and nearer the earlier one; equal fractions under different
denominators (32/64 beside 16/32, 0/64 beside 0/0), which go to the smaller core; borders whose rows are below every core of their
cluster; a row whose only edges go to rows that are no cores; two such rows joined to each other and to cores of different
clusters; degrees of exactly m and m - 1; m = 1 and m above every degree; lists whose length is not a multiple of 64; padding
entries; lists that overflow and are regrown (a first capacity of 1 edge, inside a word, one short, exactly enough); row blocks
over one list; tables of 0 and 1 rows; and random jobs with a fixed seed.
The emulator runs workgroups one after another: the races between workgroups on deg[], parent[], best_key[] and via[] are
exercised on the device only (tests/test_cluster_density_gpu.py).  One small case also runs with work-items as OS threads under
ThreadSanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emu", "cluster_density_emu_main.cpp")
INC = ["-I" + os.path.join(ROOT, "tools", "hipemu"), "-I" + os.path.join(ROOT, "mash_amd", "csrc")]
CASES = ["small", "bridge", "ties", "relabel", "noise", "degree", "lengths", "padding", "overflow"]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("emu") / "cluster_density_emu")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-DMG_HIP_EMU", "-DHIPEMU_FIBERS", *INC, SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize("case", CASES)
def test_density_kernels_on_the_cpu(emu, case):
    r = subprocess.run([emu, case], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "all cases agree" in r.stdout and "FAIL" not in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_density_kernels_on_the_cpu_random_jobs(emu):
    """`cluster_density_emu fuzz <seed> <cases>`: seed 20261021, 100 jobs: 2 .. 20 000 rows, one to three appends over one list
    (lists of up to 12 000 distinct pairs named either way round, or row blocks of a flat triangle), edges mostly inside 1 .. 40
    families with some bridges between them, counts in quarters of 64 and 32 and 0/0 (ties across denominators are common),
    m and m + 1 for an m between 1 and the mean degree + 2, every third job with a first capacity of 1 .. 5 000 edges"""
    r = subprocess.run([emu, "fuzz", "20261021", "100"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "all cases agree" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    ok = [ln for ln in r.stdout.splitlines() if ln.startswith("ok")]
    ties = [ln for ln in ok if ", 0 ties for best" not in ln]
    between = [ln for ln in ok if ", 0 between two clusters" not in ln]
    assert len(ties) >= 20 and len(between) >= 20                    # the jobs do tell the rules apart


def test_density_kernels_under_thread_sanitizer(tmp_path):
    exe = str(tmp_path / "cluster_density_emu_tsan")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=thread", "-DMG_HIP_EMU", "-pthread", *INC, SRC, "-o", exe], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("no ThreadSanitizer runtime here: " + r.stderr[-200:])
    r = subprocess.run([exe, "small"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "all cases agree" in r.stdout and "ThreadSanitizer" not in r.stderr, r.stdout[-2000:] + r.stderr[:3000]
