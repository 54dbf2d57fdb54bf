#!/usr/bin/env python
# coding: utf-8
"""Time one training batch of the sampler by its two paths — `dudf_sample_batch` (a scan of the whole shape) and
`dudf_sample_batch_indexed` (the grouped BVH walk) — over shapes of growing size, in one process on one GPU:

    python tools/bench_sampler_index.py [--batch 30000] [--reps 5] [--warmup 3] [--levels 4 5 6 7 8] [--clouds 10000 30000 100000 1000000]

Meshes: the beetle fixture (2 053 triangles) and unit icospheres / 1.1 of 20 * 4^level triangles (level 8: 1 310 720), each with a
surface cloud of 100 000 points.  Clouds (`onlyPCloud`): surface samples of the beetle.  Batch 30 000 with the recipe's percentiles
(29 970 samples: 9 990 on, 9 990 far, 9 990 near).  Per size: both paths warmed, then `reps` launches each timed by events on the
stream — median and min-max in ms —, the index build (codes, stable sort, boxes, the flag read; wall clock, median), the exact
evaluations per query of the walk, and whether the two batches are the same bits.  "auto": the smallest measured size from which
on the tree's [min, max] lies wholly below the scan's at that size and every larger one.  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from diffudf_amd import _lib, hip_ops, mesh  # noqa: E402

DEV = "cuda:0"


def icosphere(level):
    """Unit icosphere of 20 * 4^level triangles: (vertices (V,3) float64, faces (T,3) int64); every edge split at its midpoint,
    pushed onto the sphere, per level."""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g),
                  (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)], dtype=np.float64)
    f = np.array([(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
                  (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)], dtype=np.int64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    for _ in range(level):
        e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
        ue, inv = np.unique(e, axis=0, return_inverse=True)
        m = v[ue[:, 0]] + v[ue[:, 1]]
        mid = len(v) + inv.reshape(3, len(f))                      # mid[k][t]: the new vertex on edge k of face t
        v = np.concatenate([v, m / np.linalg.norm(m, axis=1, keepdims=True)])
        a, b, c = f[:, 0], f[:, 1], f[:, 2]
        f = np.concatenate([np.stack([a, mid[0], mid[2]], 1), np.stack([b, mid[1], mid[0]], 1), np.stack([c, mid[2], mid[1]], 1),
                            np.stack([mid[0], mid[1], mid[2]], 1)])
    return v, f


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Shape:
    """The arguments of one shape: tri (T,9) or None, its surface cloud, and — built here, timed — its index."""

    def __init__(self, tri, pos, nrm, reps):
        self.tri, self.pos, self.nrm = (None if tri is None else dev(tri)), dev(pos), dev(nrm)
        build = (lambda: hip_ops.cloud_index_build(self.pos)) if tri is None else (lambda: hip_ops.mesh_index_build(self.tri))
        self.index = build()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            build()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        self.build_ms = float(np.median(ts))

    def launch(self, tree, strata, step, out, stats=None):
        lib = _lib.load()
        P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        head = (P(self.tri), 0 if self.tri is None else self.tri.shape[0], P(self.pos), P(self.nrm), self.pos.shape[0], *strata, 123, step, 0, 1)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        if not tree:
            rc = lib.dudf_sample_batch(*head, *[P(t) for t in out], st)
        else:
            mi = (P(self.index), self.index.numel()) if self.tri is not None else (None, 0)
            ci = (P(self.index), self.index.numel()) if self.tri is None else (None, 0)
            rc = lib.dudf_sample_batch_indexed(*head, *mi, *ci, *[P(t) for t in out], P(stats), st)
        _lib.check(rc, "dudf_sample_batch_indexed" if tree else "dudf_sample_batch")


def time_events(fn, reps, warmup):
    """(median, min, max) in ms of fn(step), each launch between two events on the current stream."""
    for k in range(warmup):
        fn(k)
    torch.cuda.synchronize()
    ts = []
    for k in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(warmup + k)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def measure_shape(shape, strata, reps, warmup):
    n = sum(strata)
    out = [[torch.empty(n, 3, device=DEV), torch.empty(n, 3, device=DEV), torch.empty(n, device=DEV)] for _ in range(2)]
    stats = torch.zeros(1, dtype=torch.int64, device=DEV)
    shape.launch(False, strata, 0, out[0]); shape.launch(True, strata, 0, out[1], stats)
    same = all(torch.equal(a, b) for a, b in zip(*out))
    queries = strata[1] if shape.tri is None else strata[1] + strata[2]
    brute = time_events(lambda k: shape.launch(False, strata, k, out[0]), reps, warmup)
    tree = time_events(lambda k: shape.launch(True, strata, k, out[1]), reps, warmup)
    r = lambda t: [round(x, 4) for x in t]  # noqa: E731
    return {"brute_ms": r(brute), "tree_ms": r(tree), "build_ms": round(shape.build_ms, 3), "evals_per_query": round(int(stats.item()) / queries, 2),
            "identical": bool(same)}


def threshold(rows, key):
    """The smallest measured size from which on the tree's [min, max] lies wholly below the scan's; None when the largest does not."""
    best = None
    for row in sorted(rows, key=lambda r: -r[key]):
        if not row["tree_ms"][2] < row["brute_ms"][1]:
            break
        best = row[key]
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=30000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--levels", type=int, nargs="*", default=[4, 5, 6, 7, 8])
    ap.add_argument("--clouds", type=int, nargs="*", default=[10000, 30000, 100000, 1000000])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sampler_index.py: no GPU visible; nothing is measured on the CPU")
    n_on, n_off = int(args.batch * 0.333), int(args.batch * 0.666)
    strata = (n_on, n_off // 2, n_off - n_off // 2)
    bv, bf = mesh.load_obj(os.path.join(REPO, "tests", "golden", "beetle.obj"))
    bv = mesh.normalize_vertices(bv)
    rows_m = []
    for name in ["beetle"] + [f"icosphere{lv}" for lv in args.levels]:
        v, f = (bv, bf) if name == "beetle" else icosphere(int(name[9:]))
        if name != "beetle":
            v = v / 1.1
        pos, nrm = mesh.sample_surface(v, f, 100000, 123)
        shape = Shape(mesh.triangle_soup(v, f), pos, nrm, args.reps)
        rows_m.append({"mesh": name, "triangles": int(len(f)), **measure_shape(shape, strata, args.reps, args.warmup)})
        del shape
    rows_c = []
    for n in args.clouds:
        pos, nrm = mesh.sample_surface(bv, bf, n, 123)
        shape = Shape(None, pos, nrm, args.reps)
        rows_c.append({"points": int(n), **measure_shape(shape, strata, args.reps, args.warmup)})
        del shape
    print(json.dumps({"bench": "sampler_index", "device": torch.cuda.get_device_name(0), "batch": args.batch, "samples": sum(strata),
                      "reps": args.reps, "ms": "[median, min, max]", "mesh": rows_m, "cloud": rows_c,
                      "auto_min_triangles": threshold(rows_m, "triangles"), "auto_min_points": threshold(rows_c, "points")}))


if __name__ == "__main__":
    main()
