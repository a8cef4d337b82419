"""`mash triangle -H` / `mash dist -H`: what is refused is refused before a device is opened (exit status 1 and the message, on a
machine without a GPU), and the usage texts and the command summary mention the option."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASH = os.path.join(ROOT, "mash_amd", "bin", "mash")
IN = os.path.join(ROOT, "tests", "golden", "cli", "in")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    if not os.path.exists(MASH):
        g.build()
    return True


def run(*args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")       # no device, wherever this runs
    return subprocess.run([MASH, *args], capture_output=True, text=True, cwd=IN, env=env, timeout=120)


@pytest.mark.parametrize("args,other", [
    (("dist", "-H", "-t", "g1.fa", "g3.fa"), "t"),
    (("dist", "-t", "-H", "-d", "0.1", "g1.fa", "g3.fa"), "t"),
    (("dist", "-H", "-N", "3", "g1.fa", "g3.fa"), "N"),
    (("triangle", "-H", "-E", "g1.fa", "g3.fa"), "E"),
    (("triangle", "-E", "-d", "0.1", "-H", "g1.fa", "g3.fa"), "E"),
    (("triangle", "-H", "-N", "3", "g1.fa", "g3.fa"), "N"),
])
def test_spectrum_refuses_the_other_outputs(built, args, other):
    r = run(*args)
    assert r.returncode == 1 and r.stdout == ""
    assert r.stderr == f"ERROR: The option -H cannot be used with -{other}.\n"


def test_the_earlier_refusal_keeps_its_precedence_and_words(built):
    r = run("dist", "-N", "3", "-t", "-H", "g1.fa", "g3.fa")
    assert r.returncode == 1 and r.stdout == "" and r.stderr == "ERROR: The option -N cannot be used with -t.\n"


@pytest.mark.parametrize("cmd", ["dist", "triangle"])
def test_usage_lists_the_spectrum(built, cmd):
    r = run(cmd, "-h")
    assert r.returncode == 0 and " -H " in r.stdout and "-H        The distance spectrum" in r.stdout
    assert "[distance, shared-hashes, pairs, pairs at or below this distance]" in " ".join(r.stdout.split()).replace("] --", "]")


def test_command_summary_mentions_the_spectrum(built):
    r = run()
    assert r.returncode == 0
    for cmd in ("dist", "triangle"):
        ln = [x for x in r.stdout.splitlines() if x.startswith(f"  {cmd} ")]
        assert len(ln) == 1 and "(-H)" in ln[0]
