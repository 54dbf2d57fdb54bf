#!/usr/bin/env python
# coding: utf-8
"""Time the device mesh simplification (events on the stream, warmed, median of `reps` with min - max), one
configuration per process:

    python tools/bench_simplify.py --luts tests/golden/g10_meshudf.npz --size 256 --grid 64 [--oracle]
    python tools/bench_simplify.py --luts tests/golden/g10_meshudf.npz --size 512 --target-faces 50000
    python tools/bench_simplify.py --border [--cap-size 65] [--border-grid 12]

  --size N with --grid n or --target-faces t: `meshclean.simplify_mesh` on the welded Lewiner sphere mesh at N^3 (the input
    tools/bench_meshclean.py builds); beside it the three calls apart — `hip_ops.mesh_simplify` with and without the per-cell pass
    (the difference bounds its share from above: the count-only form skips it and the two emit kernels, and launches everything
    else) — the in / out counts, `fallback`, and with --oracle the numpy oracle's wall clock (tests/simplify_oracle.py) and whether
    faces and counts agree;
  --border: the open CAP-UDF sheet, welded and wound, simplified at boundary weights 0, 1 and 10, with the lattice at the
    bounding-box minimum (the default origin) and moved by half a cell: the one-sided deviation of the result's border vertices from
    the input's border edges, in units of the cell edge (mean and max).

Launches per `hip_ops.mesh_simplify` call: 2 memsets + 1 kernel (keys), the stable sort, 12 kernels (count; 11 without the per-cell
pass), 2 kernels (emit); one read-back of the eight counts.  Prints one JSON line."""
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
sys.path.insert(0, os.path.join(REPO, "tools"))

from diffudf_amd import hip_ops, marching_cubes as M, meshclean  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return {"median_ms": float(np.median(ts)), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def border_edges_of(f, n_vertices):
    return meshclean.border_edges(f, n_vertices)


def border_deviation(v_in, f_in, v_out, f_out):
    """Distances of the output's border vertices to the input's border edges (point to segment), a tensor."""
    e_in = border_edges_of(f_in, v_in.shape[0])
    e_out = border_edges_of(f_out, v_out.shape[0])
    if e_in.shape[0] == 0 or e_out.shape[0] == 0:
        return torch.zeros(0, dtype=torch.float64, device=v_in.device)
    p = v_out[torch.unique(e_out.reshape(-1))]                         # (P,3)
    a, b = v_in[e_in[:, 0]], v_in[e_in[:, 1]]                          # (E,3)
    ab = b - a
    t = (((p[:, None, :] - a[None]) * ab[None]).sum(-1) / (ab * ab).sum(-1).clamp_min(1e-300)[None]).clamp(0.0, 1.0)
    d = (p[:, None, :] - (a[None] + t[..., None] * ab[None])).norm(dim=-1)
    return d.min(1).values


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--luts", default=None)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--grid", type=int, default=None)
    ap.add_argument("--target-faces", type=int, default=None)
    ap.add_argument("--oracle", action="store_true")
    ap.add_argument("--border", action="store_true")
    ap.add_argument("--cap-size", type=int, default=65)
    ap.add_argument("--border-grid", type=int, default=12)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_simplify needs the GPU")
    dev = torch.device("cuda", 0)
    out = {"bench": "simplify", "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    if a.border:
        from test_capudf import analytic_fields
        n = a.cap_size
        ndf, vec = analytic_fields(n, "sheet")
        sv, sf = hip_ops.capudf_extract(torch.from_numpy(ndf).to(dev), torch.from_numpy(vec).to(dev), 0.008)
        v, f, _ = meshclean.clean_mesh(sv, sf, fill_holes=False)
        f = meshclean.orient_faces(v, f)
        rows = []
        lo, hi = torch.amin(v, 0), torch.amax(v, 0)
        h = float((hi - lo).max()) / a.border_grid
        # the sheet's border lies in bounding-box planes: with the default origin (the bounding-box minimum) it lies on cell faces, where
        # the containment test of the placement is decided by rounding; "centred" moves the lattice by h / 2
        for name, origin in (("bbox_min", None), ("centred", (lo - 0.5 * h).tolist())):
            for w in (0.0, 1.0, 10.0):
                ov, of, info = meshclean.simplify_mesh(v, f, cell=h, boundary_weight=w, origin=origin)
                d = border_deviation(v, f, ov, of) / info["cell"]
                rows.append({"origin": name, "boundary_weight": w, "faces": info["faces"], "fallback": info["fallback"],
                             "border_vertices": int(d.numel()), "border_deviation_mean_h": float(d.mean()) if d.numel() else 0.0,
                             "border_deviation_max_h": float(d.max()) if d.numel() else 0.0})
        out.update(config="border", cap_size=n, grid=a.border_grid, in_vertices=int(v.shape[0]), in_faces=int(f.shape[0]), weights=rows)
        print(json.dumps(out))
        return
    if (a.grid is None) == (a.target_faces is None):
        raise SystemExit("one of --grid and --target-faces")
    from bench_meshclean import sphere_soup
    if a.luts and a.luts.endswith(".npz") and "CASES" not in np.load(a.luts).files:       # the test fixture keeps them as lut_<NAME>
        z = np.load(a.luts)
        luts = {k[4:]: z[k] for k in z.files if k.startswith("lut_")}
    else:
        luts = M.load_luts(a.luts)
    sv, sf = sphere_soup(a.size, 0, dev, luts)
    v, f, _ = meshclean.clean_mesh(sv, sf, fill_holes=False)
    del sv, sf
    kw = {"grid": a.grid} if a.grid is not None else {"target_faces": a.target_faces}
    ov, of, info = meshclean.simplify_mesh(v, f, **kw)
    org, h = info["origin"], info["cell"]
    out.update(config=kw, size=a.size, in_vertices=int(v.shape[0]), in_faces=int(f.shape[0]),
               counts={k: info[k] for k in hip_ops.MESH_SIMPLIFY_COUNTS}, grid=info["grid"], count_calls=info["count_calls"],
               workspace_bytes=int(hip_ops._bytes("dudf_mesh_simplify_workspace_bytes", v.shape[0], f.shape[0])),
               simplify_mesh=timed(lambda: meshclean.simplify_mesh(v, f, **kw), a.reps, a.warmup),
               mesh_simplify=timed(lambda: hip_ops.mesh_simplify(v, f, org, h), a.reps, a.warmup),
               count_only=timed(lambda: hip_ops.mesh_simplify_count(v, f, org, h), a.reps, a.warmup))
    keys = torch.randint(0, 2 ** 40, (3 * f.shape[0],), device=dev)
    out["sort_3F_keys"] = timed(lambda: torch.sort(keys, stable=True), a.reps, a.warmup)
    out["per_cell_pass_share"] = round(max(0.0, out["mesh_simplify"]["median_ms"] - out["count_only"]["median_ms"]) / out["mesh_simplify"]["median_ms"], 3)
    if a.oracle:
        import simplify_oracle as S
        hv, hf = v.cpu().numpy(), f.cpu().numpy()
        t0 = time.perf_counter()
        want = S.simplify(hv, hf, np.array(org), h)
        out["numpy_oracle_ms"] = (time.perf_counter() - t0) * 1e3
        low = int((want["margin"] < 1e-8).sum())
        out["oracle"] = {"faces_equal": bool(np.array_equal(of.cpu().numpy(), want["faces"])),
                         "counts_equal_but_fallback": all(info[k] == want["counts"][k] for k in S.COUNT_NAMES[:7]),
                         "fallback": want["counts"]["fallback"], "cells_below_margin": low,
                         "max_position_error_h": float(np.abs(ov.cpu().numpy() - want["vertices"]).max() / h) if ov.shape[0] == len(want["vertices"]) else None}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
