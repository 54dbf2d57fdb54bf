#!/usr/bin/env python
# coding: utf-8
"""Time CAP-UDF extraction from a trained network: the dense path (`extract_fields` + `capudf_extract`) against the brick-sparse narrow
band (`extract_fields_sparse` + `SparseFields.extract`) — dense and sparse at 513^3, sparse at 1025^3 and 2049^3, dense
at 1025^3 when its 17 GB of fields can be allocated.

    python tools/bench_sparse_mc.py [--checkpoint model_best.pth --hidden 256 --layers 8] [--brick 8] [--lipschitz 1.25]
                                    [--sizes 513 1025 2049] [--reps 5] [--warmup 1] [--train-epochs 3000]

Without `--checkpoint` the configs/train_beetle.json recipe is trained in this process first (its time is reported, not part of any
figure).  Warmed, median of `reps` with min-max, events on the stream (the host read-backs of the output sizes are inside them, as a
caller pays them).  Reports, per size: candidate and stored bricks, points evaluated, the times of the coarse lattice / selection /
brick fields / CAP-UDF stages and of the whole call, `torch.cuda.max_memory_allocated`, vertex and triangle counts; at 513 also the
symmetric difference of the emitted-cell sets, dense against sparse — the one place where a learned field's coverage by the selection
bound is observed (`lipschitz` is the caller's statement, nothing verifies it).  Prints one JSON line; one process per line."""
import argparse
import contextlib
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from diffudf_amd import hip_ops, render_mc  # noqa: E402
from diffudf_amd.model import SIREN  # noqa: E402


def timed_ms(fn, reps, warmup):
    """{median, min, max} ms of fn(), events on the current stream."""
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return {"median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts))}


def trained_model(a, dev):
    hidden = [a.hidden] * a.layers
    if a.checkpoint:
        model = SIREN(3, 1, hidden, w0=30)
        model.load_state_dict(torch.load(a.checkpoint, weights_only=True))
        return model.to(dev), "tanh", 100.0, {"checkpoint": a.checkpoint}
    import train
    cfg = json.load(open(os.path.join(REPO, "configs", "train_beetle.json")))
    cfg["dataset"] = os.path.join(REPO, cfg["dataset"])
    cfg["num_epochs"] = a.train_epochs
    if a.train_epochs != 3000:                            # a shortened recipe keeps the proportions of the stages
        cfg["s1_epochs"] = a.train_epochs * 2 // 3; cfg["warmup_epochs"] = a.train_epochs // 3
    with tempfile.TemporaryDirectory() as tmp:
        cfg["checkpoint_path"] = tmp + "/"
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(sys.stderr):           # the one line on stdout is the result
            train.setup_train(cfg, dev.index or 0)
        wall = time.perf_counter() - t0
        best = [os.path.join(r, f) for r, _, fs in os.walk(tmp) for f in fs if f in ("model_best.pth", "model_final.pth")]
        best.sort(key=lambda p: not p.endswith("model_best.pth"))
        hidden = cfg["network"]["hidden_layer_nodes"]
        model = SIREN(3, 1, hidden, w0=cfg["network"]["w0"])
        model.load_state_dict(torch.load(best[0], weights_only=True))
    return model.to(dev), cfg["gt_mode"], float(cfg["alpha"]), {"trained": "configs/train_beetle.json", "epochs": a.train_epochs,
                                                               "train_wall_s": wall}


def cell_keys(cells, N):
    return (cells[:, 0] * N + cells[:, 1]) * N + cells[:, 2]


def bench_sparse(model, mode, alpha, N, a, dev):
    cfg, theta = model.hip_cfg, model.flat_parameters()
    B, thr = a.brick, a.threshold
    m, nb, nl = hip_ops.sparse_dims(N, B)
    torch.cuda.reset_peak_memory_stats()
    f = render_mc.extract_fields_sparse(model, None, N, mode, dev, alpha, threshold=thr, brick=B, lipschitz=a.lipschitz)
    v, t, cells = f.extract(want_cells=True)
    peak = torch.cuda.max_memory_allocated()
    row = {"candidate_bricks": int(f.candidate_ids.numel()), "stored_bricks": int(f.stored_ids.numel()), "cell_bricks": nb ** 3,
           "points_evaluated": (nb + 1) ** 3 + f.points_stored, "points_dense": N ** 3, "vertices": int(len(v)), "triangles": int(len(t)),
           "emitted_cells": int(len(cells)), "max_memory_allocated": int(peak)}
    # stages: the coarse lattice, the selection on it, the brick fields of the stored list, CAP-UDF on the result
    nco = (nb + 1) ** 3
    coarse = torch.empty(nco, dtype=torch.float32, device=dev)
    step = 1 << 20

    def run_coarse():
        for s in range(0, nco, step):
            hip_ops.grid_fields_lattice(cfg, theta, N, B, s, min(step, nco - s), mode, alpha, coarse)

    bound = hip_ops.sparse_bound(N, B, thr, a.lipschitz)
    per = max(1, step // B ** 3)
    S = int(f.stored_ids.numel())

    def run_bricks():
        for s in range(0, S, per):
            hip_ops.grid_fields_bricks(cfg, theta, N, B, f.stored_ids, s, min(per, S - s), mode, alpha, f.df, f.vec)

    row["ms"] = {"coarse": timed_ms(run_coarse, a.reps, a.warmup),
                 "select": timed_ms(lambda: hip_ops.sparse_select(coarse, N, B, bound), a.reps, a.warmup),
                 "brick_fields": timed_ms(run_bricks, a.reps, a.warmup),
                 "cap": timed_ms(lambda: f.extract(), a.reps, a.warmup),
                 "total": timed_ms(lambda: render_mc.extract_fields_sparse(model, None, N, mode, dev, alpha, threshold=thr, brick=B,
                                                                           lipschitz=a.lipschitz).extract(), a.reps, a.warmup)}
    return row, cell_keys(cells, N)


def bench_dense(model, mode, alpha, N, a, dev):
    thr = a.threshold
    torch.cuda.reset_peak_memory_stats()
    try:
        df, vec = render_mc.extract_fields(model, None, N, mode, dev, alpha)
    except torch.cuda.OutOfMemoryError as e:
        return {"skipped": f"allocation failed: {str(e).splitlines()[0]}"}, None
    v, t, cells = hip_ops.capudf_extract(df, vec, thr, want_cells=True)
    row = {"points_evaluated": N ** 3, "vertices": int(len(v)), "triangles": int(len(t)), "emitted_cells": int(len(cells)),
           "max_memory_allocated": int(torch.cuda.max_memory_allocated())}
    keys = cell_keys(cells, N)
    del v, t, cells
    row["ms"] = {"cap": timed_ms(lambda: hip_ops.capudf_extract(df, vec, thr), a.reps, a.warmup)}
    del df, vec
    row["ms"]["fields"] = timed_ms(lambda: render_mc.extract_fields(model, None, N, mode, dev, alpha), a.reps, a.warmup)
    row["ms"]["total"] = timed_ms(lambda: hip_ops.capudf_extract(*render_mc.extract_fields(model, None, N, mode, dev, alpha), thr),
                                  a.reps, a.warmup)
    return row, keys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--train-epochs", type=int, default=3000)
    ap.add_argument("--brick", type=int, default=8)
    ap.add_argument("--lipschitz", type=float, default=1.25)
    ap.add_argument("--threshold", type=float, default=0.008)
    ap.add_argument("--sizes", type=int, nargs="+", default=[513, 1025, 2049])
    ap.add_argument("--dense-sizes", type=int, nargs="*", default=[513, 1025])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sparse_mc needs the GPU")
    dev = torch.device("cuda", 0)
    model, mode, alpha, origin = trained_model(a, dev)
    out = {"bench": "sparse_mc", "reps": a.reps, "warmup": a.warmup, "brick": a.brick, "lipschitz": a.lipschitz, "threshold": a.threshold,
           "gt_mode": mode, "model": origin, "sizes": {}}
    for N in a.sizes:
        row = {}
        row["sparse"], ks = bench_sparse(model, mode, alpha, N, a, dev)
        if N in a.dense_sizes:
            row["dense"], kd = bench_dense(model, mode, alpha, N, a, dev)
            if kd is not None:
                both = torch.cat([ks, kd]).unique(return_counts=True)[1]
                row["emitted_cells_symmetric_difference"] = int((both == 1).sum())
                row["emitted_cells_only_dense"] = int(len(kd) - (both == 2).sum())
            del kd
        del ks
        torch.cuda.empty_cache()
        out["sizes"][str(N)] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
