# coding: utf-8
"""Oracle side of the mesh-distance tests (numpy fp64): argmin and closest point next to `oracle.sampler_oracle`'s distances,
and the meshes the tests share."""
import os
import sys

import numpy as np

from diffudf_amd import mesh
from oracle.sampler_oracle import point_triangle_dist2

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
if TOOLS not in sys.path:
    sys.path.insert(0, TOOLS)
import bench_meshdist  # noqa: E402,F401   the icosphere, and the timer and torch baseline of the speed test


def all_dist2(p, tri, chunk=512):
    """(N,T) fp64 squared distances of points p (N,3) to every triangle of tri (T,9)."""
    p = np.asarray(p, dtype=np.float64)
    return np.concatenate([point_triangle_dist2(p[i:i + chunk], tri) for i in range(0, len(p), chunk)], axis=0)


def nearest(p, tri, chunk=512):
    """(d2 (N,), idx (N,)): minimum over the triangles and the smallest index that attains it."""
    p = np.asarray(p, dtype=np.float64)
    d2 = np.empty(len(p)); idx = np.empty(len(p), dtype=np.int64)
    for i in range(0, len(p), chunk):
        m = point_triangle_dist2(p[i:i + chunk], tri)
        idx[i:i + chunk] = m.argmin(axis=1)                       # first minimum
        d2[i:i + chunk] = m.min(axis=1)
    return d2, idx


def dist2_to(p, tri_rows):
    """fp64 squared distance of point i to triangle tri_rows[i] (N,9)."""
    return np.array([point_triangle_dist2(p[i:i + 1], tri_rows[i:i + 1])[0, 0] for i in range(len(p))])


def barycentric_residual(c, tri_rows):
    """How far points c (N,3) are from lying ON their triangles tri_rows (N,9): the distance of c to the triangle."""
    return np.sqrt(dist2_to(np.asarray(c, dtype=np.float64), tri_rows))


def beetle():
    """Normalised beetle: (vertices fp64, faces, soup (2053,9) fp32)."""
    v, t = mesh.load_obj(os.path.join(GOLDEN, "beetle.obj"))
    v = mesh.normalize_vertices(v)
    return v, t, mesh.triangle_soup(v, t)


def spacing32(x):
    """fp32 spacing at |x| (x already fp32-representable or not): the bound 'one fp32 spacing'."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)
