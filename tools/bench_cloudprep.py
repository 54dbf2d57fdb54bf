#!/usr/bin/env python
# coding: utf-8
"""Time what a raw scan needs before training (`diffudf_amd.metrics.estimate_normals` / `remove_statistical_outliers`) on clouds
sampled from tests/golden/beetle.obj: the k-nearest search, the estimation kernel alone, the outlier call, the whole
`estimate_normals` (search, estimation, orientation), and beside them the same neighbourhoods composed in torch on the same GPU:
gather, batched fp64 covariance, `torch.linalg.eigh`.

    timeout -k 10 900 python tools/bench_cloudprep.py [--reps 5] [--sizes 100000,1000000] [--k 15] [--torch-rows 100000]

Warmed, median of `reps`, events on the stream, everything in this process on the same GPU.  Above 200 000 points the torch
composition is timed on the first `--torch-rows` rows only and scaled to all rows (marked "torch_scaled").  Prints one JSON line."""
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


def torch_normals(x, idx, first_row=0):
    """The neighbourhoods of rows [first_row, first_row + len(idx)) — the point itself, then its row of idx (all slots valid) — as
    torch composes them: gather, fp64 mean and covariance, `torch.linalg.eigh`, the first eigenvector."""
    own = torch.arange(first_row, first_row + idx.shape[0], device=idx.device)[:, None]
    nb = x[torch.cat([own, idx], dim=1)].double()                          # (rows, K + 1, 3)
    d = nb - nb.mean(dim=1, keepdim=True)
    cov = d.transpose(1, 2) @ d / nb.shape[1]
    lam, V = torch.linalg.eigh(cov)
    return V[:, :, 0].float(), lam


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--nb-neighbors", type=int, default=16)
    ap.add_argument("--torch-rows", type=int, default=100000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cloudprep.py: no GPU visible; nothing is measured on the CPU")
    v, t = mesh.load_obj(os.path.join(REPO, "tests", "golden", "beetle.obj"))
    v = mesh.normalize_vertices(v)
    K = args.k
    cases = []
    for n in (int(s) for s in args.sizes.split(",")):
        p, _ = mesh.sample_surface(v, t, n, seed=1)
        x = torch.from_numpy(p.astype(np.float32)).cuda()
        _, idx = metrics.knn_points(x, x, K, exclude_self=True)
        dist16, _ = metrics.knn_points(x, x, args.nb_neighbors, exclude_self=True)
        rows = n if n <= 200000 else min(n, args.torch_rows)
        ours, lam, _ = hip_ops.estimate_normals(x, idx, want_info=True)
        theirs, tlam = torch_normals(x, idx[:rows])
        dots = (ours[:rows].double() * theirs.double()).sum(dim=1).abs()
        gap = (lam[:rows, 1] - lam[:rows, 0]) >= 1e-6 * lam[:rows, 2]      # where the direction is determined
        search = time_ms(lambda: hip_ops.knn_points(x, x, K, exclude_self=True, want_dist=False), args.reps)
        est = time_ms(lambda: hip_ops.estimate_normals(x, idx), args.reps)
        est_info = time_ms(lambda: hip_ops.estimate_normals(x, idx, want_info=True), args.reps)
        outl = time_ms(lambda: hip_ops.cloud_outliers(dist16), args.reps)
        outl_all = time_ms(lambda: metrics.remove_statistical_outliers(x, args.nb_neighbors), args.reps)
        whole = time_ms(lambda: metrics.estimate_normals(x, k=K), args.reps)
        ref = time_ms(lambda: torch_normals(x, idx[:rows]), args.reps)
        scale = n / rows
        _, info = metrics.estimate_normals(x, k=K, return_info=True)
        removed = metrics.remove_statistical_outliers(x, args.nb_neighbors)[2]["removed"]
        cases.append({"n": n, "K": K, "search_ms": search, "estimate_ms": est, "estimate_with_info_ms": est_info,
                      "outliers_ms": outl, "remove_statistical_outliers_ms": outl_all, "nb_neighbors": args.nb_neighbors,
                      "outliers_removed": removed, "estimate_normals_ms": whole,
                      "components": info["orient"]["components"], "orient_rounds": info["orient"]["rounds"],
                      "torch_ms": [round(r * scale, 3) for r in ref], "torch_scaled": rows != n, "torch_rows": rows,
                      "torch_over_estimate": round(ref[0] * scale / est[0], 2),
                      "min_abs_dot_with_torch": float(dots[gap].min()), "rows_without_a_gap": int((~gap).sum()),
                      "max_eigenvalue_diff_over_lambda2": float(((lam[:rows] - tlam).abs().max(dim=1).values / tlam[:, 2]).max())})
    print(json.dumps({"bench": "cloudprep", "device": torch.cuda.get_device_name(0), "reps": args.reps,
                      "times": "[median, min, max] ms", "cases": cases}))


if __name__ == "__main__":
    main()
