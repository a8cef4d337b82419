"""The distance spectrum (`mash triangle -H`, `mash dist -H`; include/mashgpu.h: mg_compare_tri_spectrum_host) stated on the lines the
reference CLI prints: `cut -f3,5 | uniq -c` in the defined order, with the running sum.  Nothing here is computed from sketches: the
distance text is column 3 of the recording, the bin is column 5.

    order: ascending distance = descending shared-hashes fraction, compared exactly in integers (numer_a * denom_b against
           numer_b * denom_a); 0/0 -- two empty sketches, distance 0 -- orders as 1/1; equal fractions by ascending denominator
    line : <distance> TAB <numer>/<denom> TAB <pairs> TAB <pairs at or below this distance>
"""
import functools


def bin_key(numer, denom):
    """what the order compares: 0/0 stands as 1/1, and the denominator itself breaks ties"""
    return (1, 1, denom) if denom == 0 else (numer, denom, denom)


def before(a, b):
    """-1 / 0 / 1 for bins a, b given as (numer, denom)"""
    an, ad, at = bin_key(*a)
    bn, bd, bt = bin_key(*b)
    l, r = an * bd, bn * ad
    if l != r:
        return -1 if l > r else 1
    return (at > bt) - (at < bt)


def ordered(bins):
    return sorted(bins, key=functools.cmp_to_key(before))


def spectrum_of_lines(lines):
    """[(distance text, numer, denom, pairs, pairs at or below)] of `dist` / `triangle -E` lines, in the defined order"""
    count, text = {}, {}
    for ln in lines:
        f = ln.split("\t")
        numer, denom = (int(x) for x in f[4].split("/"))
        count[(numer, denom)] = count.get((numer, denom), 0) + 1
        assert text.setdefault((numer, denom), f[2]) == f[2]          # a distance is a function of the fraction
    out, below = [], 0
    for b in ordered(count):
        below += count[b]
        out.append((text[b], b[0], b[1], count[b], below))
    return out


def spectrum_stdout(stdout):
    """what -H prints where the command without it printed `stdout`"""
    return "".join(f"{d}\t{n}/{m}\t{c}\t{below}\n" for d, n, m, c, below in spectrum_of_lines(stdout.splitlines()))


def spectrum_of_counts(numer, denom):
    """(numer, denom, count) arrays in the defined order out of the {numer, denom} of every passing pair (numpy arrays)"""
    import numpy as np
    numer, denom = np.asarray(numer, dtype=np.uint64).ravel(), np.asarray(denom, dtype=np.uint64).ravel()
    keys, counts = np.unique(numer << np.uint64(32) | denom, return_counts=True)
    bins = {(int(k) >> 32, int(k) & 0xFFFFFFFF): int(c) for k, c in zip(keys, counts)}
    order = ordered(bins)
    return (np.array([b[0] for b in order], dtype=np.uint32), np.array([b[1] for b in order], dtype=np.uint32),
            np.array([bins[b] for b in order], dtype=np.uint64))
