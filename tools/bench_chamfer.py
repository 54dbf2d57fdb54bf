#!/usr/bin/env python
# coding: utf-8
"""Time the nearest-neighbour search behind `diffudf_amd.metrics.chamfer_distance` (one direction, both norms) against the
composition available without it: exact-difference `torch.cdist` in row chunks of about 1 GiB, then `min(dim=1)`.

    python tools/bench_chamfer.py [--reps 7] [--sizes 100000x100000,1000000x100000]

Points are sampled from tests/golden/beetle.obj.  Warmed, median of `reps`, events on the stream, both sides in this process on
the same GPU.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from diffudf_amd import mesh, metrics  # noqa: E402


def time_ms(fn, reps):
    fn(); torch.cuda.synchronize()                                         # warm: code objects, allocator
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def torch_nearest(x, y, norm, chunk_bytes=1 << 30, max_pairs=1 << 24):
    """What a user composes today: exact-difference `torch.cdist` in row chunks, then `min(dim=1)`.  Chunks of about 1 GiB of
    distances, further capped at `max_pairs` pairs per `cdist` call as a precaution: torch's exact-difference kernel runs one
    256-thread workgroup per pair, so 1 GiB of distances at 100 000 columns (2684 rows) is a launch of 6.9e10 threads, past the
    2^32 a HIP launch is specified for; 2^24 pairs is 2^32 threads.  Callers check this search's indices against the kernel's
    before they time it, and `max_pairs=1 << 62` gives the uncapped 1 GiB form."""
    rows = max(1, min(chunk_bytes // (4 * y.shape[0]), max_pairs // y.shape[0]))
    ds, js = [], []
    for s in range(0, x.shape[0], rows):
        if norm == 2:
            d = torch.cdist(x[s:s + rows], y, p=2.0, compute_mode='donot_use_mm_for_euclid_dist')
        else:
            d = torch.cdist(x[s:s + rows], y, p=1.0)
        v, j = d.min(dim=1)
        ds.append(v * v if norm == 2 else v); js.append(j)
    return torch.cat(ds), torch.cat(js)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="100000x100000,1000000x100000")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_chamfer.py: no GPU visible; nothing is measured on the CPU")
    v, t = mesh.load_obj(os.path.join(REPO, "tests", "golden", "beetle.obj"))
    v = mesh.normalize_vertices(v)
    cases = []
    for size in args.sizes.split(","):
        n, m = (int(s) for s in size.split("x"))
        x = torch.from_numpy(mesh.sample_surface(v, t, n, seed=1)[0]).cuda()
        y = torch.from_numpy(mesh.sample_surface(v, t, m, seed=2)[0]).cuda()
        for norm in (1, 2):
            i_hip = metrics.nearest_points(x, y, norm)[1]
            i_ref = torch_nearest(x, y, norm)[1]
            hip = time_ms(lambda: metrics.nearest_points(x, y, norm), args.reps)
            ref = time_ms(lambda: torch_nearest(x, y, norm), args.reps)
            cases.append({"n": n, "m": m, "norm": norm, "hip_ms": round(hip[0], 4), "hip_ms_min_max": [round(hip[1], 4), round(hip[2], 4)],
                          "torch_ms": round(ref[0], 3), "torch_ms_min_max": [round(ref[1], 3), round(ref[2], 3)],
                          "ratio": round(ref[0] / hip[0], 2), "pairs_per_s": round(n * m / (hip[0] * 1e-3), 0),
                          "index_agreement": float((i_hip == i_ref).float().mean())})
    print(json.dumps({"bench": "chamfer_nearest", "device": torch.cuda.get_device_name(0), "reps": args.reps, "cases": cases}))


if __name__ == "__main__":
    main()
