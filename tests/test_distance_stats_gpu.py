# coding: utf-8
"""GPU: threshold statistics of a distance vector (`metrics.distance_stats`, `dudf_distance_stats` of csrc/dudf_surfsample.hip)
against numpy (tests/surface_oracle.py `distance_stats`).  Counts, the NaN count and the maximum are integers or bit patterns:
equal.  The two sums are doubles added in another order than `math.fsum`'s exact sum: 1e-12 relative (at most 2^20 additions of
round-off 1.1e-16 each, in a tree); two calls give the same bits."""
import numpy as np
import pytest
import torch

import surface_oracle as SO
from diffudf_amd import hip_ops, metrics, synth
from diffudf_amd._lib import DudfError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = (0, 1, 255, 256, 257, 4096 * 256 + 300)


def _vector(n, seed=11):
    """Distances like a reconstruction's: most around 1e-3, a tail up to ~1."""
    u = synth.uniform01(seed, 1, 0, n)
    return (10.0 ** (-4.0 * u) * synth.uniform01(seed, 2, 0, n)).astype(np.float32)


@pytest.fixture(scope="module")
def vectors():
    return {n: _vector(n) for n in SIZES}


def _taus(d, K):
    if K == 0:
        return ()
    if K == 1:
        return (0.01,)
    present = [float(d[i]) for i in (0, len(d) // 2, len(d) - 1)] if len(d) else [0.5, 0.25, 0.125]
    # values of the vector itself (inclusive), below every value, above every value, +inf, and a spread
    return tuple(present + [-1.0, 0.0, 2.0, float("inf")] + [10.0 ** -k for k in range(1, 10)])


def _check(d, taus):
    want = SO.distance_stats(d, taus)
    counts, mx, sums = hip_ops.distance_stats(torch.from_numpy(d).to(DEV), taus)
    assert counts.dtype == torch.int64 and counts.shape == (len(taus) + 1,) and mx.dtype == torch.float32 and sums.dtype == torch.float64
    assert counts.tolist() == want["count_le"] + [want["nan"]]
    assert np.array_equal(mx.cpu().numpy().view(np.uint32), np.array([want["max"]], dtype=np.float32).view(np.uint32))
    s = sums.tolist()
    for got, ref in zip(s, (want["sum"], want["sum_sq"])):
        assert got == ref if not np.isfinite(ref) or ref == 0.0 else abs(got - ref) <= 1e-12 * abs(ref)
    again = hip_ops.distance_stats(torch.from_numpy(d).to(DEV), taus)
    assert torch.equal(again[2].view(torch.int64), sums.view(torch.int64)) and torch.equal(again[0], counts) and torch.equal(again[1], mx)
    return want


@pytest.mark.parametrize("K", [0, 1, 16])
@pytest.mark.parametrize("n", SIZES)
def test_against_numpy(vectors, n, K):
    d = vectors[n]
    taus = _taus(d, K)
    assert len(taus) == K
    want = _check(d, taus)
    if K == 16 and n:
        assert want["count_le"][0] >= 1 and want["count_le"][3] == 0 and want["count_le"][6] == n     # inclusive; below all; +inf


def test_planted_rows(vectors):
    d = vectors[257].copy()
    d[[3, 64, 200, 256]] = np.nan
    d[[0, 100, 255]] = np.inf
    d[7] = 0.0
    taus = (float(d[1]), float(np.nextafter(d[1], np.float32(0))), 0.0, float("inf"), 3.0e38)
    want = _check(d, taus)
    assert want["nan"] == 4 and want["max"] == np.inf and want["sum"] == np.inf
    assert want["count_le"][0] == want["count_le"][1] + 1 and want["count_le"][2] == 1 and want["count_le"][3] == 253 and want["count_le"][4] == 250
    # a threshold between two floats, given in double, is compared in double
    x = np.array([1.0, np.nextafter(np.float32(1.0), np.float32(2.0))], dtype=np.float32)
    assert _check(x, (1.0 + 2.0 ** -23 - 2.0 ** -30,))["count_le"] == [1]     # rounded to float32 it would admit both
    # only NaN rows: no value at all
    out = metrics.distance_stats(torch.full((300,), float("nan"), device=DEV), (1.0,))
    assert out["count_le"] == [0] and out["nan"] == 300 and out["max"] == 0.0 and np.isnan(out["mean"]) and np.isnan(out["mean_sq"])


def test_dict_surface(vectors):
    d = vectors[255]
    out = metrics.distance_stats(torch.from_numpy(d).to(DEV), (0.01, 0.1))
    want = SO.distance_stats(d, (0.01, 0.1))
    assert set(out) == {"count_le", "nan", "max", "mean", "mean_sq"}
    assert out["count_le"] == want["count_le"] and out["nan"] == 0 and out["max"] == want["max"]
    assert out["mean"] == pytest.approx(want["sum"] / 255, rel=1e-12) and out["mean_sq"] == pytest.approx(want["sum_sq"] / 255, rel=1e-12)
    empty = metrics.distance_stats(torch.empty(0, device=DEV), (0.5,))
    assert empty["count_le"] == [0] and empty["nan"] == 0 and empty["max"] == 0.0 and np.isnan(empty["mean"])


def test_refusals(vectors):
    d = torch.from_numpy(vectors[256]).to(DEV)
    with pytest.raises(DudfError, match="UNSUPPORTED"):
        metrics.distance_stats(d, tuple(0.01 * k for k in range(17)))
    with pytest.raises(DudfError):
        metrics.distance_stats(d.cpu(), (0.1,))
    with pytest.raises(DudfError):
        hip_ops.distance_stats(d.double(), (0.1,))
    assert metrics.distance_stats(d, tuple(0.01 * k for k in range(16)))["nan"] == 0
