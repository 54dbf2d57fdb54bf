# coding: utf-8
"""CPU: the numpy model of the ordered sum (tests/ordered_sum_oracle.py) is a sum — within the tolerances the GPU tests of the
summing entry points allow against `math.fsum` — and its inputs decide what tests/test_ordered_sums_gpu.py pins: for every pinned
quantity the ordered sum has other bits than numpy's pairwise sum, a left-to-right sum and a four-wave butterfly."""
import math

import numpy as np
import pytest

import cloudprep_oracle as CO
import ordered_sum_oracle as O
import surface_oracle as SO
from diffudf_amd import synth


def test_groups():
    assert [O.groups(n) for n in (0, 1, 256, 257, 65536, 65537, 10 ** 9)] == [1, 1, 1, 2, 256, 256, 256]


def test_order_by_hand():
    """One workgroup, values whose sum depends on which pair meets first."""
    h = 2.0 ** -53                                   # half an ulp of 1.0: 1 + h rounds back to 1, 1 + 2h does not
    x = np.zeros(256)
    x[0], x[128], x[64] = 1.0, h, h
    assert O.ordered_sum(x) == 1.0                   # stride 128: 1 + h = 1; stride 64: 1 + h = 1
    x[128], x[192] = 0.0, h
    assert O.ordered_sum(x) == 1.0 + 2.0 * h         # stride 128: s[64] = 2h; stride 64: 1 + 2h
    # two groups: rows 256 .. are the second partial, added after the first
    y = np.zeros(257)
    y[0], y[1], y[256] = 1.0, h, h
    assert O.ordered_sum(y) == 1.0 and O.left_to_right_sum(y[[1, 256, 0]]) == 1.0 + 2.0 * h
    # a second trip: thread 0 of group 0 takes rows 0 and 65536 before any tree
    z = np.zeros(65793)
    z[0], z[65536], z[1] = h, h, 1.0
    assert O.ordered_sum(z) == 1.0 + 2.0 * h
    z[65536], z[65537] = 0.0, h                      # ... thread 1 takes rows 1 and 65537: 1 + h = 1, then + h again
    assert O.ordered_sum(z) == 1.0


@pytest.mark.parametrize("n", [1, 255, 257, 1000, 65793, 4096 * 256 + 300])
def test_is_a_sum(n):
    """1e-13 relative to the exact sum: the tightest of the tolerances of test_distance_stats_gpu (1e-12), test_surface_sample_gpu
    (1e-13) and test_cloudprep_gpu (1e-12)."""
    u = synth.uniform01(11, 1, 0, n)
    for x in ((10.0 ** (-4.0 * u) * synth.uniform01(11, 2, 0, n)).astype(np.float32).astype(np.float64), u, u * u):
        ref = math.fsum(x.tolist())
        assert abs(O.ordered_sum(x) - ref) <= 1e-13 * abs(ref)
    assert O.ordered_sum(np.arange(n, dtype=np.float64)) == n * (n - 1) / 2          # integers: exact in every order


def test_skipped_and_special_rows():
    assert O.ordered_sum([]) == 0.0 and O.bits(O.ordered_sum([])) == 0
    assert O.ordered_sum([1.0, np.inf, 2.0]) == np.inf and np.isnan(O.ordered_sum([np.inf, -np.inf]))


def _pinned(n):
    d = O.distance_vector(n).astype(np.float64)
    m = CO.outliers(O.knn_distances(n))["mean_dist"]
    fin = np.isfinite(m)
    mu = O.outlier_statistics(m, 2.0)[0]
    c = np.where(fin, m, mu) - mu
    return {"sum of distances": d, "sum of squared distances": d * d, "face norms": SO.face_terms(*O.triangles(n))[1],
            "mean distances": np.where(fin, m, 0.0), "centred squares": c * c}


@pytest.mark.parametrize("n", O.SIZES[1:])
def test_inputs_tell_the_orders_apart(n):
    for name, x in _pinned(n).items():
        want = O.bits(O.ordered_sum(x))
        for order in (O.pairwise_sum, O.left_to_right_sum, O.butterfly_sum):
            assert O.bits(order(x)) != want, (name, order.__name__)


def test_outlier_statistics_follow_the_sum():
    """mu, sigma and the threshold move with the order of the two sums behind them, and equal the plain oracle's to rounding."""
    for n in O.SIZES[1:]:
        kd = O.knn_distances(n)
        ref = CO.outliers(kd, 2.0)
        mu, sigma, thr = O.outlier_statistics(ref["mean_dist"], 2.0)
        for got, want in ((mu, ref["mean"]), (sigma, ref["std"]), (thr, ref["threshold"])):
            assert abs(got - want) <= 1e-12 * abs(want)
        assert O.outlier_statistics(ref["mean_dist"], 2.0, total=O.left_to_right_sum)[0] != mu
    one = O.outlier_statistics(CO.outliers(O.knn_distances(1))["mean_dist"], 2.0)
    assert one[1] == 0.0 and one[2] == one[0] > 0.0
