#!/usr/bin/env python
# coding: utf-8
"""Time the device mesh clean-up (`meshclean.clean_mesh`: weld, prune, fill holes, rounds to a fixed point; events on the stream)
beside its numpy oracle (tests/meshclean_oracle.py, wall clock) on one mesh: the closed device-marching-cubes mesh of a sphere
volume, un-indexed into a soup with V = 3 F, with a few faces removed (so there is welding and hole filling to do).

    python tools/bench_meshclean.py --luts tests/golden/g10_meshudf.npz [--size 256] [--drop 16] [--reps 5] [--warmup 2]

The Lewiner tables are an input, as for tools/bench_mcsdf.py.  Warmed, median of `reps`; the device time includes the one read-back
of the counts per round.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from diffudf_amd import hip_ops, marching_cubes as M, meshclean  # noqa: E402
import meshclean_oracle as O  # noqa: E402


def sphere_soup(N, drop, dev, luts):
    """(vertices (3F,3) float64, faces (F,3) int64) on `dev`: every face of the sphere's mesh with its own three vertices, every
    `len // drop`-th face left out."""
    g = torch.linspace(-1.0, 1.0, N, device=dev)
    vol = (torch.sqrt((g[:, None, None] - 0.013) ** 2 + (g[None, :, None] + 0.021) ** 2 + (g[None, None, :] - 0.017) ** 2) - 0.6).contiguous()
    data, offs, dims = M._pack_luts(luts)
    v, f, _, _ = hip_ops.mc_lewiner_extract(vol, 0.0, torch.from_numpy(data).to(dev), offs, dims)
    f = f.long()
    if drop > 0:
        keep = torch.ones(f.shape[0], dtype=torch.bool, device=dev)
        keep[::max(1, f.shape[0] // drop)] = False
        f = f[keep]
    soup = v.double()[f.reshape(-1)] * (2.0 / (N - 1)) - 1.0
    return soup.contiguous(), torch.arange(soup.shape[0], device=dev, dtype=torch.int64).reshape(-1, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--luts", default=None)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--drop", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_meshclean needs the GPU")
    dev = torch.device("cuda", 0)
    if a.luts and a.luts.endswith(".npz") and "CASES" not in np.load(a.luts).files:       # the test fixture keeps them as lut_<NAME>
        z = np.load(a.luts)
        luts = {k[4:]: z[k] for k in z.files if k.startswith("lut_")}
    else:
        luts = M.load_luts(a.luts)
    v, f = sphere_soup(a.size, a.drop, dev, luts)
    cv, cf, info = meshclean.clean_mesh(v, f)
    for _ in range(a.warmup):
        meshclean.clean_mesh(v, f)
    ts = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); meshclean.clean_mesh(v, f); e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    hv, hf = v.cpu().numpy(), f.cpu().numpy()
    hs = []
    for i in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        ov, of, oinfo = O.clean(hv, hf)
        if i >= a.warmup:
            hs.append((time.perf_counter() - t0) * 1e3)
    same = bool(cv.cpu().numpy().tobytes() == ov.tobytes() and np.array_equal(cf.cpu().numpy(), of) and info == oinfo)
    print(json.dumps({"bench": "meshclean", "size": a.size, "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
                      "soup_vertices": int(v.shape[0]), "soup_faces": int(f.shape[0]), "info": info, "equals_oracle": same,
                      "workspace_bytes": int(hip_ops._bytes("dudf_mesh_clean_workspace_bytes", v.shape[0], f.shape[0])),
                      "device_clean_ms": float(np.median(ts)), "device_clean_ms_all": [round(t, 3) for t in ts],
                      "numpy_oracle_ms": float(np.median(hs))}))


if __name__ == "__main__":
    main()
