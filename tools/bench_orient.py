#!/usr/bin/env python
# coding: utf-8
"""Time the K-nearest search and the normal orientation behind `diffudf_amd.metrics.orient_normals` on clouds sampled from
tests/golden/beetle.obj: the cell-list search against the brute scan (same bits, so the ratio is pure search cost) and against the
composition available without either, exact-difference `torch.cdist` in row chunks + `topk`; the cell-list build alone; the
orientation with its rounds and launches.

    timeout -k 10 900 python tools/bench_orient.py [--reps 5] [--sizes 100000,1000000] [--k 10] [--torch-rows 20000]

Warmed, median of `reps`, events on the stream, everything in this process on the same GPU.  Above 200 000 points the torch
composition is timed on the first `--torch-rows` query rows only and scaled to all rows (marked "torch_scaled"): it is O(n m).
Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from diffudf_amd import hip_ops, mesh, metrics  # noqa: E402


def time_ms(fn, reps):
    fn(); torch.cuda.synchronize()                                         # warm: code objects, allocator
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b))
    return [round(float(np.median(ts)), 4), round(float(min(ts)), 4), round(float(max(ts)), 4)]


def torch_knn(x, y, K, first_row=0, max_pairs=1 << 24):
    """Exact-difference `torch.cdist` in row chunks of at most 2^24 pairs (one workgroup per pair: bench_chamfer.py), the row's own
    column masked, then `topk`."""
    rows = max(1, max_pairs // y.shape[0])
    ds, js = [], []
    for s in range(0, x.shape[0], rows):
        d = torch.cdist(x[s:s + rows], y, p=2.0, compute_mode='donot_use_mm_for_euclid_dist')
        r = torch.arange(d.shape[0], device=d.device)
        d[r, r + s + first_row] = float("inf")
        v, j = torch.topk(d, K, dim=1, largest=False)
        ds.append(v * v); js.append(j)
    return torch.cat(ds), torch.cat(js)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--torch-rows", type=int, default=20000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_orient.py: no GPU visible; nothing is measured on the CPU")
    v, t = mesh.load_obj(os.path.join(REPO, "tests", "golden", "beetle.obj"))
    v = mesh.normalize_vertices(v)
    K = args.k
    cases = []
    for n in (int(s) for s in args.sizes.split(",")):
        p, nrm = mesh.sample_surface(v, t, n, seed=1)
        sign = np.where(np.random.default_rng(0).random(n) < 0.5, -1.0, 1.0)[:, None]
        x = torch.from_numpy(p.astype(np.float32)).cuda(); nr = torch.from_numpy((nrm * sign).astype(np.float32)).cuda()
        dg, ig = metrics.knn_points(x, x, K, exclude_self=True)
        db, ib = metrics.knn_points(x, x, K, exclude_self=True, brute=True)
        same = bool(torch.equal(dg.view(torch.int32), db.view(torch.int32)) and torch.equal(ig, ib))
        rows = n if n <= 200000 else min(n, args.torch_rows)
        it = torch_knn(x[:rows], x, K)[1]
        grid = time_ms(lambda: metrics.knn_points(x, x, K, exclude_self=True), args.reps)
        brute = time_ms(lambda: metrics.knn_points(x, x, K, exclude_self=True, brute=True), args.reps)
        build = time_ms(lambda: hip_ops.knn_grid_build(x), args.reps)
        ref = time_ms(lambda: torch_knn(x[:rows], x, K), args.reps)
        scale = n / rows
        stats = {}

        def orient():
            stats.update(hip_ops.orient_normals(x, nr, ig)[4])
        ori = time_ms(orient, args.reps)
        counts = hip_ops.orient_normals(x, nr, ig)[3].tolist()
        cases.append({"n": n, "K": K, "grid_equals_brute": same, "grid_ms": grid, "brute_ms": brute, "grid_build_ms": build,
                      "brute_over_grid": round(brute[0] / grid[0], 2),
                      "torch_ms": [round(r * scale, 3) for r in ref], "torch_scaled": rows != n, "torch_rows": rows,
                      "torch_over_grid": round(ref[0] * scale / grid[0], 2),
                      "torch_index_agreement": float((it == ig[:rows]).float().mean()),
                      "orient_ms": ori, "orient_rounds": stats.get("rounds"), "orient_launches": stats.get("launches"),
                      "components": counts[0], "forest_edges": counts[1]})
    print(json.dumps({"bench": "orient_normals", "device": torch.cuda.get_device_name(0), "reps": args.reps,
                      "times": "[median, min, max] ms", "cases": cases}))


if __name__ == "__main__":
    main()
