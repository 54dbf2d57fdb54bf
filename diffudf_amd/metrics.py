# coding: utf-8
"""Chamfer distance and normal consistency on the device — the part of `pytorch3d.loss.chamfer_distance` that reference
cuantitative.py:10-19 uses (pytorch3d is a CUDA extension), and the vertex normals open3d computes for it at :99-100.

The nearest-neighbour search, the sums behind the means and the vertex normals are HIP kernels (csrc/dudf_chamfer.hip);
there is no CPU path: CPU tensors raise DudfError."""
import torch

from . import hip_ops
from ._lib import DudfError


def nearest_points(x, y, norm=2):
    """(dist (n,) float32, idx (n,) int64): for every row of x (n,3) its nearest row of y (m,3) — the `dists[..., 0]` and
    `idx[..., 0]` of pytorch3d's `knn_points(x[None], y[None], norm=norm, K=1)`.  norm 2: squared Euclidean; norm 1: L1."""
    return hip_ops.nearest_points(x, y, norm)


def _batched(t, what):
    if not torch.is_tensor(t):
        raise DudfError(f"chamfer_distance: {what} must be a tensor; got {type(t).__name__}")
    if t.device.type != "cuda":
        raise DudfError(f"chamfer_distance: {what} must live on the GPU (got {t.device}); there is no CPU fallback")
    if t.dim() == 2:
        t = t[None]
    if t.dim() != 3 or t.shape[2] != 3:
        raise DudfError(f"chamfer_distance: {what} must have shape (N, P, 3) or (P, 3); got {tuple(t.shape)}")
    return t.float()


def chamfer_distance(x, y, x_normals=None, y_normals=None, norm=2):
    """`pytorch3d.loss.chamfer_distance(x, y, x_normals=, y_normals=, norm=)` with its default reductions (point and batch
    reduction "mean", both directions, `abs_cosine=True`): returns (cham_dist, cham_normals), 0-dim float32 tensors on the input
    device; cham_normals is None without normals.  Per batch element  cham_dist = sum_x d(x, y) / P1 + sum_y d(y, x) / P2  with
    d the squared Euclidean (norm 2) or L1 (norm 1) distance to the nearest point, cham_normals the same sum of the two
    directions' means of 1 - |cos(normal, normal of the nearest point)|; both averaged over the batch.
    x, y: (N, P, 3) or (P, 3).  The other pytorch3d keywords (lengths, weights, reductions, single_directional, ...) are not
    accepted."""
    if norm not in (1, 2):
        raise ValueError("Support for 1 or 2 norm.")
    x, y = _batched(x, "x"), _batched(y, "y")
    if x.shape[0] != y.shape[0]:
        raise ValueError("x and y must have the same batch size")
    if (x_normals is None) != (y_normals is None):
        raise ValueError("x_normals and y_normals must be given together")
    have_n = x_normals is not None
    if have_n:
        x_normals, y_normals = _batched(x_normals, "x_normals"), _batched(y_normals, "y_normals")
        if x_normals.shape != x.shape or y_normals.shape != y.shape:
            raise ValueError("normals must have the shape of their points")
    N, P1, P2 = x.shape[0], x.shape[1], y.shape[1]
    if N == 0 or P1 == 0 or P2 == 0:
        raise ValueError("chamfer_distance: empty point set")
    sums = torch.zeros(N, 2, 2, dtype=torch.float64, device=x.device)           # [batch][direction][distance, normal term]
    for b in range(N):
        for d, (p, q, pn, qn) in enumerate(((x[b], y[b], x_normals[b] if have_n else None, y_normals[b] if have_n else None),
                                            (y[b], x[b], y_normals[b] if have_n else None, x_normals[b] if have_n else None))):
            dist, idx = hip_ops.nearest_points(p, q, norm, want_idx=have_n)
            hip_ops.chamfer_terms(dist, idx, pn, qn, out=sums[b, d])
    means = sums / torch.tensor([P1, P2], dtype=torch.float64, device=x.device)[None, :, None]
    per_batch = means.sum(dim=1)                                                 # (N, 2): x -> y plus y -> x
    out = per_batch.mean(dim=0).float()
    return out[0], (out[1] if have_n else None)


def vertex_normals(vertices, faces):
    """(V,3) float32 CUDA tensor: area-weighted unit vertex normals (open3d `compute_vertex_normals(normalized=True)`).
    vertices (V,3), faces (F,3): CUDA tensors."""
    return hip_ops.vertex_normals(vertices, faces)
