#!/usr/bin/env python
# coding: utf-8
"""Time the device mesh topology (events on the stream, warmed, median of `reps`):
  - `meshclean.face_topology` (winding, components, integer areas) on the welded Lewiner sphere meshes tools/bench_meshclean.py builds,
    with half of the windings reversed at random, and the whole `finish="mesh"` chain (soup -> `clean_mesh(fill_holes=False)` ->
    `orient_faces`) on their soups;
  - the same chain on the CAP-UDF soup of an analytic sheet, beside the numpy oracles on the host (tests/meshclean_oracle.py,
    tests/meshtopo_oracle.py, wall clock), with the comparison of the two results.

    python tools/bench_meshtopo.py --luts tests/golden/g10_meshudf.npz [--sizes 256,512] [--cap-size 65] [--reps 5] [--warmup 2]

The device times include the read-backs (one word per Borůvka round, the counts).  Prints one JSON line."""
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
from bench_meshclean import sphere_soup  # noqa: E402
import meshclean_oracle as O  # noqa: E402
import meshtopo_oracle as T  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), [round(t, 3) for t in ts]


def chain(v, f):
    cv, cf, _ = meshclean.clean_mesh(v, f, fill_holes=False)
    return cv, meshclean.orient_faces(cv, cf)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--luts", default=None)
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--cap-size", type=int, default=65)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_meshtopo needs the GPU")
    dev = torch.device("cuda", 0)
    if a.luts and a.luts.endswith(".npz") and "CASES" not in np.load(a.luts).files:       # the test fixture keeps them as lut_<NAME>
        z = np.load(a.luts)
        luts = {k[4:]: z[k] for k in z.files if k.startswith("lut_")}
    else:
        luts = M.load_luts(a.luts)
    out = {"bench": "meshtopo", "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "spheres": []}
    for N in [int(s) for s in a.sizes.split(",") if s]:
        sv, sf = sphere_soup(N, 0, dev, luts)
        v, f, _ = meshclean.clean_mesh(sv, sf, fill_holes=False)
        turn = torch.from_numpy(np.random.default_rng(N).random(f.shape[0]) < 0.5).to(dev)
        g = torch.where(turn[:, None], f[:, [0, 2, 1]], f).contiguous()
        topo = meshclean.face_topology(g, v.shape[0], v)
        t_topo, all_topo = timed(lambda: meshclean.face_topology(g, v.shape[0], v), a.reps, a.warmup)
        t_chain, all_chain = timed(lambda: chain(sv, sf), a.reps, a.warmup)
        out["spheres"].append({"size": N, "vertices": int(v.shape[0]), "faces": int(f.shape[0]),
                               "counts": {k: topo[k] for k in hip_ops.MESH_TOPOLOGY_COUNTS}, "area": float(topo["area"].sum()),
                               "workspace_bytes": int(hip_ops._bytes("dudf_mesh_topology_workspace_bytes", f.shape[0])),
                               "face_topology_ms": t_topo, "face_topology_ms_all": all_topo,
                               "finish_mesh_chain_ms": t_chain, "finish_mesh_chain_ms_all": all_chain})
    from test_capudf import analytic_fields
    n = a.cap_size
    ndf, vec = analytic_fields(n, "sheet")
    cv0, cf0 = hip_ops.capudf_extract(torch.from_numpy(ndf).to(dev), torch.from_numpy(vec).to(dev), 0.008)
    gv, gf = chain(cv0, cf0)
    t_cap, all_cap = timed(lambda: chain(cv0, cf0), a.reps, a.warmup)
    hv, hf = cv0.cpu().numpy(), cf0.cpu().numpy()
    hs = []
    for i in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        ov, of, _ = O.clean(hv, hf, fill=False)
        want = T.topology(of, len(ov), ov)
        if i >= a.warmup:
            hs.append((time.perf_counter() - t0) * 1e3)
    out["cap_sheet"] = {"size": n, "soup_vertices": int(cv0.shape[0]), "soup_faces": int(cf0.shape[0]), "faces": int(gf.shape[0]),
                        "counts": {k: want[k] for k in T.COUNT_NAMES},
                        "equals_oracle": bool(gv.cpu().numpy().tobytes() == ov.tobytes() and np.array_equal(gf.cpu().numpy(), want["faces"])),
                        "finish_mesh_chain_ms": t_cap, "finish_mesh_chain_ms_all": all_cap, "numpy_oracle_ms": float(np.median(hs))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
