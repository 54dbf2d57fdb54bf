# coding: utf-8
"""GPU: K nearest neighbours (diffudf_amd.metrics.knn_points, csrc/dudf_orient.hip) — the cell-list search against the brute scan bit
for bit, K = 1 against `nearest_points` bit for bit, and the brute scan against the float64 oracle of tests/orient_oracle.py.

Tolerances (u = 2^-24), every row checked:
  distances  the sorted fp32 distance at position k is within 8u (relative) of the oracle's at k — the bound test_chamfer_gpu.py derives
             for one pair (each difference one rounding, square and three-term sum at most four more: 5u, 8u with room); it carries
             over position by position because sorting is monotone: if every entry of a list moves by at most a factor (1 +- e), so
             does its k-th smallest;
  indices    in range, distinct within a row, never the row itself with exclude_self; the float64 distance at the returned index k
             within 16u of the oracle's k-th."""
import numpy as np
import pytest
import torch

import orient_oracle as OO
from diffudf_amd import hip_ops, metrics

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DEV = "cuda:0"


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def both(x, y, K, exclude_self):
    """(dist, idx) of the cell-list search after checking that the brute scan returns the same bits."""
    dg, ig = metrics.knn_points(_cuda(x), _cuda(y), K, exclude_self=exclude_self)
    db, ib = metrics.knn_points(_cuda(x), _cuda(y), K, exclude_self=exclude_self, brute=True)
    assert dg.dtype == torch.float32 and ig.dtype == torch.int64 and dg.shape == ig.shape == (len(x), K)
    dg, ig, db, ib = dg.cpu().numpy(), ig.cpu().numpy(), db.cpu().numpy(), ib.cpu().numpy()
    assert np.array_equal(dg.view(np.uint32), db.view(np.uint32)), "grid and brute distances differ"
    assert np.array_equal(ig, ib), "grid and brute indices differ"
    return db, ib


def check(x, y, K, exclude_self, what, oracle=None):
    """oracle: `OO.knn(x, y, 16, exclude_self, exact=True)` computed once for several K (its first K columns are the answer for K)."""
    dist, idx = both(x, y, K, exclude_self)
    n, m = len(x), len(y)
    d64, i64 = oracle if oracle is not None else OO.knn(x, y, K, exclude_self, exact=True)
    d64, i64 = d64[:, :K], i64[:, :K]
    pad = ~np.isfinite(d64)
    assert np.array_equal(idx == -1, pad) and np.array_equal(np.isinf(dist), pad), what       # padding exactly where the oracle pads
    real = ~pad
    assert (idx[real] >= 0).all() and (idx[real] < m).all(), what
    with np.errstate(invalid="ignore"):                         # inf - inf at the padded places, which `real` leaves out
        err = np.abs(dist.astype(np.float64) - d64)[real]
    worst = float((err / np.maximum(d64[real], 1e-300)).max()) if real.any() else 0.0
    print(f"{what}: max |d_k - oracle_k| / oracle_k = {worst / U:.3f} u over {n} rows x {K}")
    assert (err <= 8 * U * d64[real]).all(), (what, worst / U)
    rows = np.repeat(np.arange(n)[:, None], K, axis=1)
    at = OO.pair_distance(x[rows[real]], y[idx[real]])
    over = float(((at - d64[real]) / np.maximum(d64[real], 1e-300)).max()) if real.any() else 0.0
    print(f"{what}: float64 distance at the returned index exceeds the oracle's k-th by at most {over / U:.3f} u")
    assert (np.abs(at - d64[real]) <= 16 * U * d64[real]).all(), (what, over / U)
    if exclude_self:
        assert (idx != rows).all(), what
    srt = np.sort(np.where(real, idx, -1 - np.arange(K)[None, :]), axis=1)                   # distinct within a row (pads made distinct)
    assert (srt[:, 1:] != srt[:, :-1]).all(), what
    key = (dist.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (idx.astype(np.uint64) & np.uint64(0xffffffff))
    assert (key[:, 1:] > key[:, :-1])[real[:, 1:]].all(), what                               # ascending by (distance, index)
    return dist, idx


@pytest.mark.parametrize("K", [1, 10, 16])
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1025])
def test_random_cloud_on_itself(n, K):
    x = (np.random.default_rng(n).random((n, 3)) * 2 - 1).astype(np.float32)
    for exclude_self in (False, True):
        dist, idx = check(x, x, K, exclude_self, f"n = m = {n}, K = {K}, exclude_self = {exclude_self}")
        if not exclude_self:
            assert (dist[:, 0] == 0).all() and (idx[:, 0] == np.arange(n)).all()


def test_k1_equals_nearest_points_bit_for_bit():
    rng = np.random.default_rng(7)
    for n, m in ((1025, 257), (3000, 2000), (1, 1)):
        x = (rng.random((n, 3)) * 2 - 1).astype(np.float32); y = (rng.random((m, 3)) * 2 - 1).astype(np.float32)
        d1, i1 = hip_ops.nearest_points(_cuda(x), _cuda(y))
        for brute in (False, True):
            d, i = metrics.knn_points(_cuda(x), _cuda(y), 1, brute=brute)
            assert torch.equal(d[:, 0].view(torch.int32), d1.view(torch.int32)) and torch.equal(i[:, 0], i1), (n, m, brute)


@pytest.mark.parametrize("K", [1, 10, 16])
def test_queries_outside_the_box_of_y(K):
    rng = np.random.default_rng(11)
    x = (rng.random((3000, 3)) * 2 - 1).astype(np.float32)
    x[::7] *= 3.0; x[5] = (40.0, -2.0, 0.5); x[6] = (-1e6, 1e6, 3.0)
    y = (rng.random((2000, 3)) - 0.5).astype(np.float32)
    check(x, y, K, False, f"3000 x 2000, K = {K}")


@pytest.mark.parametrize("K", [1, 10, 16])
def test_lattice_of_ties(K):
    x = OO.lattice(12, 1.0 / 8.0)
    for exclude_self in (False, True):
        check(x, x, K, exclude_self, f"12^3 lattice, K = {K}, exclude_self = {exclude_self}")


def test_duplicates_and_outliers():
    rng = np.random.default_rng(13)
    five = (rng.random((5, 3)) * 0.01).astype(np.float32)
    out = rng.normal(size=(10, 3))
    out = (out / np.linalg.norm(out, axis=1, keepdims=True)).astype(np.float32)
    x = np.concatenate([np.tile(five, (2000, 1)), out]).astype(np.float32)
    x = x[rng.permutation(len(x))]
    oracle = OO.knn(x, x, 16, True, exact=True)
    for K in (10, 16):
        check(x, x, K, True, f"2000 x 5 duplicates + 10 outliers, K = {K}", oracle)


def test_fewer_candidates_than_k():
    rng = np.random.default_rng(17)
    for m, K, exclude_self in ((1, 1, True), (3, 10, False), (3, 3, True), (11, 16, True), (16, 16, True)):
        x = rng.random((m, 3)).astype(np.float32)
        check(x, x, K, exclude_self, f"m = {m}, K = {K}, exclude_self = {exclude_self}")
    y = rng.random((40, 3)).astype(np.float32)
    y[3] = np.nan; y[8, 1] = np.inf                                 # rows that are never returned
    x = rng.random((50, 3)).astype(np.float32)
    dist, idx = check(x, y, 16, False, "non-finite rows of y")
    assert not np.isin(idx, (3, 8)).any()
    x[4, 2] = np.nan                                                # a row of x that has no answer
    dist, idx = both(x, y, 4, False)
    assert np.isnan(dist[4]).all() and (idx[4] == -1).all() and np.isfinite(dist[np.arange(50) != 4]).all()


def test_repeated_calls_and_refusals():
    x = (np.random.default_rng(19).random((1025, 3))).astype(np.float32)
    a = metrics.knn_points(_cuda(x), _cuda(x), 10, exclude_self=True)
    b = metrics.knn_points(_cuda(x), _cuda(x), 10, exclude_self=True)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    d, i = metrics.knn_points(torch.zeros(0, 3, device=DEV), _cuda(x), 4)
    assert d.shape == (0, 4) and i.shape == (0, 4)
    from diffudf_amd._lib import DudfError
    for K in (0, 17):
        with pytest.raises(DudfError):
            metrics.knn_points(_cuda(x), _cuda(x), K)
    with pytest.raises(DudfError):
        metrics.knn_points(torch.from_numpy(x), torch.from_numpy(x), 4)          # CPU tensors: there is no CPU path
