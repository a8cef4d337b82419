"""What `mash within` computes, in plain Python (test infrastructure; no device, no library).

containSketches (CommandContain.cpp:231-263) walks the reference's and the query's ascending hash lists with two pointers;
`walk` is that loop, `closed` the closed form the device implements.  `j_min` turns the -e threshold into the smallest query
count j that passes, `line` formats one output line as the reference's `cout << double` does (6 significant digits), and
`output` is the whole stdout of a run from the sketches."""
import math
import struct


def walk(ref, qry):
    """the serial walk: (common, j).  ref, qry: ascending sequences of distinct integers"""
    common = 0
    denom = min(len(ref), len(qry))
    i = j = 0
    steps = 0
    while steps < denom and i < len(ref):
        if ref[i] < qry[j]:
            i += 1
            continue                      # (steps-- undoes the loop's steps++)
        if qry[j] < ref[i]:
            j += 1
        else:
            i += 1
            j += 1
            common += 1
        steps += 1
    return common, j


def closed(ref, qry):
    """the closed form: c = #{q <= max(R)}, j = min(|R|, |Q|, c), common = #(Q[:j] & R)"""
    if not len(ref) or not len(qry):
        return 0, 0
    top = ref[-1]
    c = sum(1 for q in qry if q <= top)
    j = min(len(ref), len(qry), c)
    members = set(ref)
    return sum(1 for q in qry[:j] if q in members), j


def termination(ref, qry):
    """which condition ends the walk: 'Q' (j reached |Q| <= |R|), 'R' (j reached |R| < |Q|), 'exhausted' (R ran out with
    c < min(|R|, |Q|)), or 'empty'"""
    if not len(ref) or not len(qry):
        return "empty"
    _, j = closed(ref, qry)
    if j < min(len(ref), len(qry)):
        return "exhausted"
    return "Q" if len(qry) <= len(ref) else "R"


def as_float(x):
    """(double)(float)x: the threshold is handed to writeOutput as a float (CommandContain.cpp:167, :179)"""
    return struct.unpack("f", struct.pack("f", x))[0]


def error_bound(j):
    return 1.0 / math.sqrt(j) if j else math.inf


def j_min(max_error):
    """the smallest j >= 1 with 1 / sqrt(j) <= max_error; None: no j passes (max_error <= 0 or NaN)"""
    if not max_error > 0:
        return None
    if max_error >= 1:
        return 1
    j = max(1, math.ceil(1.0 / (max_error * max_error)))
    while j > 1 and error_bound(j - 1) <= max_error:
        j -= 1
    while not error_bound(j) <= max_error:
        j += 1
    return j


def passes(j, max_error):
    return j >= 1 and error_bound(j) <= max_error


def fmt(x):
    """`cout << double` at the default precision"""
    return "%g" % x


def line(common, j, ref_name, qry_name):
    return "%s\t%s\t%s\t%s\n" % (fmt(common / j), fmt(error_bound(j)), ref_name, qry_name)


def output(refs, queries, e):
    """stdout of `mash within -e <e>`: refs, queries = [(name, ascending hashes)]; query-major, only error <= (float)e"""
    thr = as_float(e)
    out = []
    for qn, qh in queries:
        for rn, rh in refs:
            common, j = closed(rh, qh)
            if passes(j, thr):
                out.append(line(common, j, rn, qn))
    return "".join(out)


def parse(text):
    """recorded lines -> [(score text, error text, reference, query)]"""
    return [tuple(l.split("\t")) for l in text.splitlines()]
