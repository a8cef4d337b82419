"""tests/golden/within as the within tests read it: the cases of cases.json, their inputs sketched by the CPU oracle, and the
stdout tests/within_model.py expects for a case.  Test infrastructure; no device.

A .msh input of the fixture is the reference CLI's `mash sketch -i` of one of the two FASTA files at the sketch size cases.json
names, so its sketches are the oracle's of that file at that size -- cut to the run's sketch size where they are larger
(Sketch.cpp:162-165: "Its sketches will be reduced"), kept as they are where they are smaller (:150, the containment rule)."""
import gzip
import json
import os

from tests import within_model as wm

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "within")


def load_cases():
    return json.load(open(os.path.join(DIR, "cases.json")))


def recorded(name):
    return open(os.path.join(DIR, name + ".out")).read()


def read_fasta(path):
    """[(name, sequence)]: the name is the header's first word"""
    recs = []
    with gzip.open(path, "rb") as f:
        for l in f.read().splitlines():
            if l.startswith(b">"):
                recs.append([l[1:].split()[0].decode(), []])
            else:
                recs[-1][1].append(l)
    return [(n, b"".join(s)) for n, s in recs]


_orc = None


def sketch_fasta(path, k, s, individual, name=None):
    """[(name, ascending hashes as ints)] of a FASTA file: one sketch per sequence of at least k bases (-i, Sketch.cpp:337-341),
    or one of the whole file under the name it was given by"""
    global _orc
    if _orc is None:
        from oracle import pyoracle
        _orc = pyoracle.Oracle()
    p = _orc.params(k=k, s=s)
    recs = [(n, q) for n, q in read_fasta(path) if len(q) >= k]
    groups = [(n, [q]) for n, q in recs] if individual else [(name or os.path.basename(path), [q for _, q in recs])]
    return [(n, [int(x) for x in _orc.sketch_records(qs, p)[0]]) for n, qs in groups]


def case_inputs(case, meta):
    """(refs, queries, e, refused) of a case: what its command line reads, as [(name, hashes)]"""
    args = case["cmd"][1:]
    flags = {"-i": False, "-l": False, "-a": False, "-n": False}
    vals = {"-e": "0.05", "-s": "1000", "-k": None, "-p": None, "-z": None}
    files = []
    it = iter(args)
    for a in it:
        if a in flags:
            flags[a] = True
        elif a in vals:
            vals[a] = next(it)
        else:
            files.append(a)
    k = meta["k"]
    ref_is_msh = files[0].endswith(".msh")
    refused = ref_is_msh and (vals["-k"] is not None or flags["-n"])           # CommandContain.cpp:61-71; -a and -z go on (:73-81)
    s_run = meta["sketches"][files[0][:-4]]["s"] if ref_is_msh else int(vals["-s"])

    def load(f, individual):
        if f.endswith(".msh"):
            sk = meta["sketches"][f[:-4]]
            return [(n, h[:s_run]) for n, h in sketch_fasta(os.path.join(DIR, sk["source"]), k, sk["s"], True)]
        return sketch_fasta(os.path.join(DIR, f), k, s_run, individual, name=f)

    queries = []
    for f in files[1:]:
        for g in (meta["lists"][f] if flags["-l"] else [f]):
            queries += load(g, flags["-i"])
    return load(files[0], flags["-i"]), queries, float(vals["-e"]), refused


def model_stdout(case, meta):
    refs, queries, e, refused = case_inputs(case, meta)
    return "" if refused else wm.output(refs, queries, e)
