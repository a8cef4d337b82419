"""bench.py --dump-outputs on the CPU: dump_outputs() fed with a triangle the oracle computed writes every pair (small
triangle) or the same seeded sample of pairs in every run (large triangle), in reference order, as float32 / float64
.npy files within the size limit, with the sums over all pairs."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _triangle(oracle, n):
    from workloads import synth
    table, nh, ln = synth.clustered_sketches(n, 200, clusters=5, seed=4, pool=300, private=80)
    numer, denom, _, _ = oracle.triangle(table, nh, ln, 0, n, 21, 4.0 ** 21)
    out = torch.from_numpy(np.stack([numer, denom], 1).astype(np.int32))
    return out, numer.astype(np.int64), denom.astype(np.int64)


def _load(d):
    return {k: np.load(os.path.join(d, k + ".npy")) for k in ("pair_index", "numer", "denom", "sums")}


def test_dump_writes_every_pair_of_a_small_triangle(oracle, tmp_path):
    n = 90
    out, numer, denom = _triangle(oracle, n)
    pairs = n * (n - 1) // 2
    bench.dump_outputs(str(tmp_path), out, 0, n, pairs, "cpu", 1, 0)
    d = _load(tmp_path)
    assert d["numer"].dtype == np.float32 and d["denom"].dtype == np.float32 and d["pair_index"].dtype == np.float64
    assert np.array_equal(d["pair_index"], np.arange(pairs))
    assert np.array_equal(d["numer"], numer) and np.array_equal(d["denom"], denom)
    assert list(d["sums"]) == [numer.sum(), denom.sum()] and d["sums"].dtype == np.float64


def test_dump_samples_the_same_pairs_every_run(oracle, tmp_path, monkeypatch):
    n = 90
    out, numer, denom = _triangle(oracle, n)
    pairs = n * (n - 1) // 2
    monkeypatch.setattr(bench, "DUMP_PAIRS", 500)
    bench.dump_outputs(str(tmp_path / "a"), out, 0, n, pairs, "cpu", 1, 0)
    bench.dump_outputs(str(tmp_path / "b"), out.clone(), 0, n, pairs, "cpu", 1, 0)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    idx = a["pair_index"].astype(np.int64)
    assert 450 < len(idx) <= 500 and np.all(np.diff(idx) > 0) and idx[-1] < pairs
    assert np.array_equal(a["numer"], numer[idx]) and np.array_equal(a["denom"], denom[idx])
    assert list(a["sums"]) == [numer.sum(), denom.sum()]


def test_dump_of_the_headline_size_stays_within_64_mb():
    assert bench.DUMP_PAIRS * (4 + 4 + 8) + 4 * 128 <= 64 * 1024 * 1024
