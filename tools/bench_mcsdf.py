#!/usr/bin/env python
# coding: utf-8
"""Time Lewiner's marching cubes of a signed volume: the device kernels (`dudf_mc_lewiner_count` + `_emit`, events on the stream),
the host library on the same volume (`dudf_mc_lewiner_run`, wall clock), and `get_mesh_sdf` end to end (grid values + extraction,
wall clock ending in a device synchronise), at 256^3 and 512^3 of a sphere-like field.

    python tools/bench_mcsdf.py --luts tests/golden/g10_meshudf.npz [--sizes 256 512] [--reps 5] [--warmup 2] [--hidden 256 --layers 8]

The Lewiner tables are an input (`--luts`: an .npz of them or the reference's table module; default: `marching_cubes.load_luts()`).
Warmed, median of `reps`, all sides in this process (the serial host library too: seconds per run at 512^3).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from diffudf_amd import hip_ops, marching_cubes as M, render_mc, synth  # noqa: E402
from diffudf_amd.model import SIREN  # noqa: E402


def sphere_field(N, dev):
    g = torch.linspace(-1.0, 1.0, N, device=dev)
    return (torch.sqrt((g[:, None, None] - 0.013) ** 2 + (g[None, :, None] + 0.021) ** 2 + (g[None, None, :] - 0.017) ** 2) - 0.6).contiguous()


def median_events_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def median_wall_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--luts", default=None)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--layers", type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mcsdf needs the GPU")
    dev = torch.device("cuda", 0)
    if a.luts and a.luts.endswith(".npz") and "CASES" not in np.load(a.luts).files:       # the test fixture keeps them as lut_<NAME>
        z = np.load(a.luts)
        luts = {k[4:]: z[k] for k in z.files if k.startswith("lut_")}
    else:
        luts = M.load_luts(a.luts)
    data, offs, dims = M._pack_luts(luts)
    lut_dev = torch.from_numpy(data).to(dev)
    hidden = [a.hidden] * a.layers
    model = SIREN(3, 1, hidden, w0=30).to(dev)
    with torch.no_grad():
        model.flat_parameters().copy_(torch.from_numpy(synth.flatten_params(synth.siren_params(hidden, seed=123))).to(dev))
    out = {"bench": "mcsdf", "reps": a.reps, "warmup": a.warmup, "network": f"{a.layers}x{a.hidden}", "sizes": {}}
    for N in a.sizes:
        vol = sphere_field(N, dev)
        v, f, _, _ = hip_ops.mc_lewiner_extract(vol, 0.0, lut_dev, offs, dims)
        row = {"vertices": int(v.shape[0]), "triangles": int(f.shape[0])}
        row["device_count_emit_ms"] = median_events_ms(lambda: hip_ops.mc_lewiner_extract(vol, 0.0, lut_dev, offs, dims), a.reps, a.warmup)
        host_vol = vol.cpu().numpy()
        row["host_library_ms"] = median_wall_ms(lambda: M.marching_cubes_sdf(host_vol, 0.0, luts, raw_normals=True), a.reps, a.warmup)
        row["get_mesh_sdf_ms"] = median_wall_ms(lambda: render_mc.get_mesh_sdf(model, N=N, device=dev, max_batch=1 << 20, luts=luts),
                                                a.reps, a.warmup)
        row["grid_values_ms"] = median_events_ms(lambda: render_mc.sdf_grid_values(model, N, dev, 1 << 20), a.reps, a.warmup)
        out["sizes"][str(N)] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
