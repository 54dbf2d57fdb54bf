#!/usr/bin/env python
# coding: utf-8
"""Time the mesh-distance query of `diffudf_amd.metrics.MeshIndex` — index build, query through the index, the same entry point's
brute-force mode — against the composition available without it: the same closest-point arithmetic written with torch ops in
fp64, in row chunks so that no intermediate exceeds 1 GiB.

    python tools/bench_meshdist.py [--level 5] [--queries 65536] [--reps 5] [--warmup 2]

Mesh: the unit icosphere of the tests (level 5: T = 20 480); queries uniform in [-1,1]^3.  Warmed, median of `reps`, device
synchronised, all sides in this process on the same GPU.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from diffudf_amd import mesh, metrics, synth  # noqa: E402


def time_ms(fn, reps=5, warmup=2):
    """Median wall time in ms of fn(), each run ending in a device synchronise."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def icosphere(level=5):
    """Unit icosphere, 20 * 4^level triangles (level 5: 20 480): (vertices (V,3) float64, faces (T,3) int64)."""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g),
         (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(x, dtype=np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        cache, nf = {}, []

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m)); cache[k] = len(v) - 1
            return cache[k]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.asarray(v), np.asarray(f, dtype=np.int64)


def icosphere_soup(level=5):
    """(T,9) float32 soup of the unit icosphere."""
    return mesh.triangle_soup(*icosphere(level))


def uniform_queries(n, seed=5):
    return np.stack([synth.uniform01(seed, 700 + k, 0, n) * 2.0 - 1.0 for k in range(3)], axis=1).astype(np.float32)


def torch_mesh_distance(points, tri, chunk_bytes=1 << 30):
    """The torch baseline: (dist (Q,) float32, idx (Q,) int64).  Closest point by the Voronoi regions of every triangle, fp64,
    component-wise (Q_chunk, T) tensors of at most `chunk_bytes` each."""
    T = tri.shape[0]
    t = tri.double()
    a = [t[None, :, k] for k in range(3)]
    ab = [t[None, :, 3 + k] - a[k] for k in range(3)]
    ac = [t[None, :, 6 + k] - a[k] for k in range(3)]
    dot = lambda u, v: u[0] * v[0] + u[1] * v[1] + u[2] * v[2]   # noqa: E731
    rows = max(1, chunk_bytes // (8 * T))
    ds, js = [], []
    for s in range(0, points.shape[0], rows):
        p = points[s:s + rows].double()
        ap = [p[:, k, None] - a[k] for k in range(3)]
        d1, d2 = dot(ab, ap), dot(ac, ap)
        bp = [ap[k] - ab[k] for k in range(3)]
        d3, d4 = dot(ab, bp), dot(ac, bp)
        cp = [ap[k] - ac[k] for k in range(3)]
        d5, d6 = dot(ab, cp), dot(ac, cp)
        va, vb, vc = d3 * d6 - d5 * d4, d5 * d2 - d1 * d6, d1 * d4 - d3 * d2
        den = 1.0 / (va + vb + vc)
        v, w = vb * den, vc * den                                   # interior; the regions below overwrite it, vertex a last
        t_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        m_bc = (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)
        v, w = torch.where(m_bc, 1.0 - t_bc, v), torch.where(m_bc, t_bc, w)
        m_ac = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
        v, w = torch.where(m_ac, 0.0, v), torch.where(m_ac, d2 / (d2 - d6), w)
        m_c = (d6 >= 0) & (d5 <= d6)
        v, w = torch.where(m_c, 0.0, v), torch.where(m_c, 1.0, w)
        m_ab = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
        v, w = torch.where(m_ab, d1 / (d1 - d3), v), torch.where(m_ab, 0.0, w)
        m_b = (d3 >= 0) & (d4 <= d3)
        v, w = torch.where(m_b, 1.0, v), torch.where(m_b, 0.0, w)
        m_a = (d1 <= 0) & (d2 <= 0)
        v, w = torch.where(m_a, 0.0, v), torch.where(m_a, 0.0, w)
        r = [ap[k] - (ab[k] * v + ac[k] * w) for k in range(3)]
        best, j = dot(r, r).min(dim=1)
        ds.append(torch.sqrt(best).float()); js.append(j)
    return torch.cat(ds), torch.cat(js)


def measure(level=5, queries=65536, reps=5, warmup=2, baseline_reps=None, baseline_warmup=None):
    """dict of the four times (ms) and what they were taken on."""
    if not torch.cuda.is_available():
        raise SystemExit("bench_meshdist.py: no GPU visible; nothing is measured on the CPU")
    tri = torch.from_numpy(icosphere_soup(level)).cuda()
    pts = torch.from_numpy(uniform_queries(queries)).cuda()
    scene = metrics.MeshIndex.from_soup(tri)
    d_idx = scene.distance(pts)
    d_ref, _ = torch_mesh_distance(pts[:4096], tri)
    build = time_ms(lambda: metrics.MeshIndex.from_soup(tri), reps, warmup)
    indexed = time_ms(lambda: scene.distance(pts), reps, warmup)
    brute = time_ms(lambda: scene.distance(pts, brute=True), reps, warmup)
    base = time_ms(lambda: torch_mesh_distance(pts, tri), baseline_reps or reps, warmup if baseline_warmup is None else baseline_warmup)
    return {"bench": "mesh_distance", "device": torch.cuda.get_device_name(0), "triangles": int(tri.shape[0]), "queries": int(queries),
            "reps": reps, "index_build_ms": round(build, 4), "query_indexed_ms": round(indexed, 4), "query_brute_ms": round(brute, 4),
            "torch_fp64_ms": round(base, 3), "ratio_torch_over_indexed": round(base / indexed, 2),
            "max_abs_diff_vs_torch": float((d_idx[:4096] - d_ref).abs().max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--level", type=int, default=5)
    ap.add_argument("--queries", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    print(json.dumps(measure(args.level, args.queries, args.reps, args.warmup)))


if __name__ == "__main__":
    main()
