# coding: utf-8
"""Float64 restatement of what diffudf_amd/metrics.py computes (pytorch3d's `knn_points(K=1)` / `chamfer_distance` with default
reductions and open3d's area-weighted vertex normals), for tests/test_chamfer_cpu.py and tests/test_chamfer_gpu.py.

The nearest-neighbour search is brute force on exact differences in float64, chunked over the rows of x; it runs on whatever
torch device it is given (the CPU for the pinning test against scipy's cKDTree, the GPU for the 100 000-point cases, where float64
torch arithmetic is the independent implementation the HIP kernel is held against)."""
import numpy as np
import torch


def pair_distance(a, b, norm):
    """float64 distance of matching rows: squared Euclidean (norm 2) or L1 (norm 1) — pytorch3d's `dists`."""
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return (d * d).sum(-1) if norm == 2 else np.abs(d).sum(-1)


def nearest(x, y, norm, device="cpu", chunk_bytes=1 << 29):
    """(d1 (n,) float64, i1 (n,) int64, d2 (n,) float64): nearest distance, the SMALLEST index that attains it, and the nearest
    distance among the other rows of y (inf when y has one row)."""
    assert norm in (1, 2)
    xt = torch.as_tensor(np.asarray(x), device=device).double()
    yt = torch.as_tensor(np.asarray(y), device=device).double()
    n, m = xt.shape[0], yt.shape[0]
    rows = max(1, int(chunk_bytes // (8 * 3 * max(m, 1))))
    ar = torch.arange(m, device=device)
    d1 = torch.empty(n, dtype=torch.float64, device=device); d2 = torch.empty_like(d1)
    i1 = torch.empty(n, dtype=torch.int64, device=device)
    for s in range(0, n, rows):
        diff = xt[s:s + rows, None, :] - yt[None, :, :]
        d = (diff * diff).sum(-1) if norm == 2 else diff.abs().sum(-1)
        del diff
        lo = d.min(dim=1).values
        idx = torch.where(d == lo[:, None], ar[None, :], m).min(dim=1).values
        d.scatter_(1, idx[:, None], float("inf"))
        d1[s:s + rows], i1[s:s + rows], d2[s:s + rows] = lo, idx, d.min(dim=1).values
        del d
    return d1.cpu().numpy(), i1.cpu().numpy(), d2.cpu().numpy()


def normal_term(x_normals, y_normals, idx, eps=1e-6):
    """1 - |cos(x_normals[p], y_normals[idx[p]])| per row, cos = a.b / (max(|a|, eps) max(|b|, eps)) (`F.cosine_similarity`)."""
    a = np.asarray(x_normals, dtype=np.float64); b = np.asarray(y_normals, dtype=np.float64)[np.asarray(idx)]
    na = np.maximum(np.sqrt((a * a).sum(-1)), eps); nb = np.maximum(np.sqrt((b * b).sum(-1)), eps)
    return 1.0 - np.abs((a * b).sum(-1) / (na * nb))


def chamfer(x, y, norm, x_normals=None, y_normals=None, idx_xy=None, idx_yx=None, device="cpu"):
    """(cham_dist, cham_normals) of ONE pair of clouds, float64: sum_x d / P1 + sum_y d / P2 and the same for the normal term.
    idx_xy / idx_yx: evaluate the normal term at these neighbour indices instead of the oracle's own (near-ties)."""
    dxy, ixy, _ = nearest(x, y, norm, device)
    dyx, iyx, _ = nearest(y, x, norm, device)
    cd = dxy.mean() + dyx.mean()
    if x_normals is None:
        return cd, None
    nc = normal_term(x_normals, y_normals, ixy if idx_xy is None else idx_xy).mean() + \
        normal_term(y_normals, x_normals, iyx if idx_yx is None else idx_yx).mean()
    return cd, nc


def vertex_normals(vertices, faces):
    """(V,3) float64: every face adds (v1 - v0) x (v2 - v0) to its three vertices (faces with an index outside [0, V) are
    skipped), then normalise; a zero sum gives (0, 0, 1)."""
    v = np.asarray(vertices, dtype=np.float64); f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    f = f[((f >= 0) & (f < len(v))).all(1)]
    c = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    acc = np.zeros_like(v)
    for k in range(3):
        np.add.at(acc, f[:, k], c)
    ln = np.sqrt((acc * acc).sum(1))
    out = np.tile(np.array([0.0, 0.0, 1.0]), (len(v), 1))
    ok = ln > 0
    out[ok] = acc[ok] / ln[ok, None]
    return out
