#!/usr/bin/env python
# coding: utf-8
"""Time the fused march against a mesh (`MeshIndex.trace_rays`, one launch) against the same loop composed from
`MeshIndex.distance` and torch masking (reference src/render_st.py:255-268: per iteration a compaction of the live rays — whose size
the host has to read —, a distance query, the masked update), and `MeshIndex.occupancy` through the index against its brute-force
mode.

    python tools/bench_meshtrace.py [--size 512] [--level 5] [--queries 65536] [--reps 5] [--warmup 2]

Rays: generate_st's set-up for a size x size image (camera and field of view of configs/st_beetle_gt.json; 120 degrees for the
sphere so that part of the rays miss it).  Meshes: the unit icosphere (level 5: T = 20 480) and the normalised beetle of
tests/golden.  Warmed, median of `reps`, HIP events on the stream around each run (the composed loop's host reads are inside).
Both marches are checked to give the same positions, hits and masks.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_meshdist  # noqa: E402
from diffudf_amd import hip_ops, mesh, metrics  # noqa: E402

CAMERA = [1.6, 1.2, 2.4]
BOUND = 1.3


def event_ms(fn, reps=5, warmup=2, before=None):
    """Median time in ms of fn(*before()) between two events on the current stream; before() runs outside the timed region."""
    ts = []
    for i in range(warmup + reps):
        args = before() if before else ()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(*args)
        b.record()
        b.synchronize()
        if i >= warmup:
            ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def setup_rays(size, fov, device="cuda:0"):
    import generate_st
    return hip_ops.render_setup_rays(size, size, fov, 0.5, generate_st.camera_rotation(CAMERA), CAMERA, [1, -1, 1, -1, 1, -1], device)


def composed_march(scene, rays, t0, mask, surface_eps=0.001, max_iterations=30, bound=BOUND):
    """The reference loop with `MeshIndex.distance` as its query and torch ops for the rest; t0 and mask in place, returns hits."""
    hits = torch.zeros_like(mask)
    for _ in range(max_iterations):
        live = mask.nonzero().squeeze(1)                    # the host reads its size
        if live.numel() == 0:
            break
        d = scene.distance(t0[live].float())
        t0[live] = t0[live] + rays[live] * d.double()[:, None]
        hit = d < surface_eps
        hits[live] = hits[live] | hit.to(torch.uint8)
        mask[live] = mask[live] & (~hit).to(torch.uint8)
        mask &= ((t0 > -bound) & (t0 < bound)).all(dim=1).to(torch.uint8)
    return hits


def measure_march(scene, size, fov, reps=5, warmup=2, surface_eps=0.001, max_iterations=30):
    rays, t0, mask = setup_rays(size, fov)
    fresh = lambda: (t0.clone(), mask.clone())                                     # noqa: E731
    ta, ma = fresh(); tb, mb = fresh()
    ha = scene.trace_rays(rays, ta, ma, surface_eps, max_iterations, BOUND)
    hb = composed_march(scene, rays, tb, mb, surface_eps, max_iterations, BOUND)
    same = bool(torch.equal(ha, hb) and torch.equal(ma, mb) and torch.equal(ta, tb))
    fused = event_ms(lambda a, b: scene.trace_rays(rays, a, b, surface_eps, max_iterations, BOUND), reps, warmup, fresh)
    composed = event_ms(lambda a, b: composed_march(scene, rays, a, b, surface_eps, max_iterations, BOUND), reps, warmup, fresh)
    return {"rays": int(size * size), "valid": int(mask.sum()), "hits": int(ha.sum()), "same_result": same,
            "fused_ms": round(fused, 4), "composed_ms": round(composed, 3), "ratio_composed_over_fused": round(composed / fused, 2)}


def sphere_scene(level):
    return metrics.MeshIndex.from_soup(torch.from_numpy(bench_meshdist.icosphere_soup(level)).cuda())


def beetle_scene():
    v, f = mesh.load_obj(os.path.join(REPO, "tests", "golden", "beetle.obj"))
    return metrics.MeshIndex(mesh.normalize_vertices(v), f, device="cuda:0")


def measure_occupancy(scene, queries, reps=5, warmup=2):
    pts = torch.from_numpy(bench_meshdist.uniform_queries(queries)).cuda()
    same = bool(torch.equal(scene.occupancy(pts, return_count=True)[1], scene.occupancy(pts, return_count=True, brute=True)[1]))
    indexed = event_ms(lambda: scene.occupancy(pts), reps, warmup)
    brute = event_ms(lambda: scene.occupancy(pts, brute=True), reps, warmup)
    return {"queries": int(queries), "same_counts": same, "indexed_ms": round(indexed, 4), "brute_ms": round(brute, 4),
            "ratio_brute_over_indexed": round(brute / indexed, 2)}


def measure(size=512, level=5, queries=65536, reps=5, warmup=2, parts=("sphere", "beetle", "occupancy")):
    if not torch.cuda.is_available():
        raise SystemExit("bench_meshtrace.py: no GPU visible; nothing is measured on the CPU")
    out = {"bench": "mesh_trace", "device": torch.cuda.get_device_name(0), "reps": reps}
    sphere = sphere_scene(level) if ("sphere" in parts or "occupancy" in parts) else None
    if "sphere" in parts:
        out["sphere"] = dict(measure_march(sphere, size, 120, reps, warmup), triangles=int(sphere.tri.shape[0]))
    if "beetle" in parts:
        b = beetle_scene()
        out["beetle"] = dict(measure_march(b, size, 45, reps, warmup), triangles=int(b.tri.shape[0]))
    if "occupancy" in parts:
        out["occupancy"] = dict(measure_occupancy(sphere, queries, reps, warmup), triangles=int(sphere.tri.shape[0]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--level", type=int, default=5)
    ap.add_argument("--queries", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    print(json.dumps(measure(args.size, args.level, args.queries, args.reps, args.warmup)))


if __name__ == "__main__":
    main()
