# coding: utf-8
"""GPU: the double sums of the geometry entry points are the ordered sum of csrc/dudf_ordsum.h, bit for bit — against its numpy
model (tests/ordered_sum_oracle.py), on inputs that tell the orders apart (tests/test_ordered_sum_cpu.py).  Pinned: both sums of
`distance_stats`, the distance sum of `chamfer_terms`, `metrics.surface_area`, and mu, sigma and the threshold of `cloud_outliers`.
The normal-consistency sum of `chamfer_terms` is not: its products are contracted and numpy cannot form them."""
import numpy as np
import pytest
import torch

import ordered_sum_oracle as O
import surface_oracle as SO
from diffudf_amd import hip_ops, metrics

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STD_RATIO = 1.5


def _same_bits(name, got, want):
    print(f"{name}: device {float(got)!r} ({O.bits(got):#018x}), ordered sum {float(want)!r} ({O.bits(want):#018x})")
    assert O.bits(got) == O.bits(want), name


@pytest.mark.parametrize("n", O.SIZES)
def test_distance_stats_sums(n):
    d = O.distance_vector(n)
    sums = hip_ops.distance_stats(torch.from_numpy(d).to(DEV), ())[2].tolist()
    d64 = d.astype(np.float64)
    _same_bits("sum d", sums[0], O.ordered_sum(d64))
    _same_bits("sum d*d", sums[1], O.ordered_sum(d64 * d64))         # the product rounded, then added: contraction is off in that unit


@pytest.mark.parametrize("n", O.SIZES)
def test_chamfer_terms_distance_sum(n):
    d = O.distance_vector(n)
    out = hip_ops.chamfer_terms(torch.from_numpy(d).to(DEV), None).tolist()
    _same_bits("sum dist", out[0], O.ordered_sum(d.astype(np.float64)))
    assert out[1] == 0.0


@pytest.mark.parametrize("n", O.SIZES)
def test_surface_area(n):
    v, f = O.triangles(n)
    _same_bits("area", metrics.surface_area(v, f), 0.5 * O.ordered_sum(SO.face_terms(v, f)[1]))


@pytest.mark.parametrize("n", O.SIZES)
def test_cloud_outlier_statistics(n):
    kd = torch.from_numpy(O.knn_distances(n)).to(DEV)
    mean, _, stats, _, _ = hip_ops.cloud_outliers(kd, STD_RATIO)
    m = mean.cpu().numpy()
    assert np.isfinite(m).sum() == (n - 1 if n >= 255 else n)
    mu, sigma, thr = O.outlier_statistics(m, STD_RATIO)
    got = stats.tolist()
    _same_bits("mu", got[0], mu)
    _same_bits("sigma", got[1], sigma)
    _same_bits("threshold", got[2], thr)
