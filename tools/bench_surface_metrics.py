#!/usr/bin/env python
# coding: utf-8
"""Time the device surface sampler and one `surface_metrics` call (`diffudf_amd.metrics`, csrc/dudf_surfsample.hip).

    python tools/bench_surface_metrics.py [--reps 5] [--warmup 2] [--rings 332]

The mesh is a latitude-longitude sphere of 2 * rings^2 faces (332: 220 448, what marching cubes gives for a sphere at 256^3).
`sample_surface` at 100 000 and 1 000 000 samples next to the host sampler `mesh.sample_surface` (wall clock, numpy), and one
`surface_metrics` call with 100 000 samples against a 100 000-point cloud of the same sphere.  Device times: `warmup` unrecorded
calls, then the median of `reps`, events on the stream.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from diffudf_amd import hip_ops, mesh, metrics, synth  # noqa: E402


def time_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b))
    return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(float(min(ts)), 4), "max_ms": round(float(max(ts)), 4)}


def host_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(float(min(ts)), 3), "max_ms": round(float(max(ts)), 3)}


def sphere_mesh(rings, radius=0.8):
    """(vertices float64, faces int64) CUDA tensors: a latitude-longitude sphere of `rings` x `rings` quads split in two —
    rings = 332 gives 220 448 faces, the face count of a marching-cubes sphere on a 256^3 lattice.  The faces shrink towards the
    poles, where one triangle of every quad collapses."""
    th = torch.linspace(0.0, np.pi, rings + 1, dtype=torch.float64, device="cuda:0")
    ph = torch.linspace(0.0, 2.0 * np.pi, rings + 1, dtype=torch.float64, device="cuda:0")
    T, P = torch.meshgrid(th, ph, indexing="ij")
    v = radius * torch.stack([torch.sin(T) * torch.cos(P), torch.sin(T) * torch.sin(P), torch.cos(T)], dim=-1).reshape(-1, 3)
    i, j = torch.meshgrid(torch.arange(rings, device="cuda:0"), torch.arange(rings, device="cuda:0"), indexing="ij")
    p = (i * (rings + 1) + j).reshape(-1)
    f = torch.cat([torch.stack([p, p + rings + 1, p + rings + 2], dim=1), torch.stack([p, p + rings + 2, p + 1], dim=1)])
    return v.contiguous(), f.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rings", type=int, default=332)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_surface_metrics.py: no GPU visible; nothing is measured on the CPU")
    v, f = sphere_mesh(args.rings)
    hv, hf = v.cpu().numpy(), f.cpu().numpy()
    out = {"bench": "surface_metrics", "device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
           "faces": int(f.shape[0]), "vertices": int(v.shape[0]), "sample_surface": []}
    for n in (100000, 1000000):
        dev = time_ms(lambda: hip_ops.mesh_sample_surface(v, f, n, seed=1), args.reps, args.warmup)
        host = host_ms(lambda: mesh.sample_surface(hv, hf, n, seed=1), args.reps)
        out["sample_surface"].append({"n": n, "device": dev, "host_numpy": host, "ratio": round(host["median_ms"] / dev["median_ms"], 1)})
    d = np.stack([synth.normal01(7, k, 0, 100000) for k in range(3)], axis=1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    cloud = torch.from_numpy((0.8 * d).astype(np.float32)).cuda()
    normals = torch.from_numpy(d.astype(np.float32)).cuda()
    for mode in (True, False):
        res = metrics.surface_metrics(v, f, cloud, normals, n_samples=100000, point_to_surface=mode)
        t = time_ms(lambda: metrics.surface_metrics(v, f, cloud, normals, n_samples=100000, point_to_surface=mode), args.reps, args.warmup)
        out["surface_metrics_point_to_surface" if mode else "surface_metrics_sample_to_sample"] = {
            "n_samples": 100000, "cloud": 100000, **t, "chamfer_l1": res["chamfer_l1"], "fscore_0.005": res["fscore"][0.005]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
