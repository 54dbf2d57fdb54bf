# coding: utf-8
"""Which kernels does a fixed list of calls launch?  One process walks queries, training steps, weight gradients by layer range
and a ray-march iteration over widths, depths, batch sizes and the options that select kernels, and writes — per sweep / GEMM
call — the kernel name dudf_debug_kernel_choice predicts (when the library has it).  Run it under the profiler with two builds
and compare the traces:
    rocprofv3 --kernel-trace --output-format csv -d OUT/a -o a -- python tools/launch_census.py run OUT/pred_a.json   (DUDF_LIB=old build)
    rocprofv3 --kernel-trace --output-format csv -d OUT/b -o b -- python tools/launch_census.py run OUT/pred_b.json
    python tools/launch_census.py compare OUT/a OUT/b OUT/pred_b.json
`compare`: the two ordered lists of (kernel name, grid, workgroup, LDS bytes) must be identical, and every predicted name must be
the traced sweep / GEMM kernel at its place.  A group of calls whose workspace would exceed MAX_WS_BYTES is left out and named in the
output (a 29 970-point training workspace of a 70-layer 512-wide network would take 70 GB)."""
import csv
import ctypes
import glob
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WIDTHS, DEPTHS, SIZES = (32, 64, 128, 256, 512), (1, 2, 8, 34, 70), (1, 17, 29970)
SINGLES = ({}, {"pair_launch": 0}, {"split_quads": 0}, {"split": 0}, {"sweep_family": 0}, {"wgrad_family": 1}, {"wgrad_family": 2},
           {"wgrad_tr": 1}, {"wgrad_buffers": 3}, {"deterministic": 1})
PAIR, WGRAD, QUERY = 16, -1, 16          # dudf_debug_kernel_choice: which | PAIR, which = WGRAD, flags | QUERY
S, C, TRAIN, HAVE_E = 1, 2, 4, 8
MAX_WS_BYTES = 12 << 30


def run(pred_path):
    import numpy as np
    import torch
    from diffudf_amd import _lib, hip_ops as hip, synth
    if not hasattr(ctypes.CDLL(_lib.LIB_PATH), "dudf_debug_kernel_choice"):      # the older build of an A/B pair
        del _lib.SYMBOLS["dudf_debug_kernel_choice"]
    lib = _lib.load()
    can_predict = "dudf_debug_kernel_choice" in _lib.SYMBOLS
    pred, buf = [], ctypes.create_string_buffer(128)

    def choice(cfg, n, nh, which, flags):
        rc = lib.dudf_debug_kernel_choice(ctypes.byref(cfg), n, nh, which, flags, buf, len(buf))
        return rc, buf.value.decode()

    def expect(cfg, n, nh, seq, query=0):
        """seq: (sweep, flags) per run_sweep; the quads and the plain columns share one grid where a pair kernel exists"""
        if not can_predict:
            return
        for base, flags in seq:
            flags |= query
            if nh > 0 and n > nh and base < 4:
                rc, name = choice(cfg, n, nh, base | PAIR, flags)
                if rc == 0:
                    pred.append(name)
                    continue
            for which in ([base + 4] if nh > 0 and base < 4 else []) + ([base] if n > nh or nh == 0 or base == 8 else []):
                rc, name = choice(cfg, n, nh, which, flags)
                assert rc == 0, (cfg.hidden, cfg.n_hidden_layers, n, nh, which, flags, rc)
                pred.append(name)

    def expect_wgrad(cfg, n, nh):
        if can_predict and cfg.n_hidden_layers >= 2:
            rc, name = choice(cfg, n, nh, WGRAD, 0)
            assert rc == 0, (cfg.hidden, cfg.n_hidden_layers, n, nh, rc)
            pred.append(name)

    dev = torch.device("cuda", 0)
    ones = torch.ones(4, device=dev)
    w_eik, w_hess = [1e4, 1e4, 0.0, 1e3], [1e4, 1e4, 1e4, 1e3]
    all_flags = S | C | TRAIN | HAVE_E
    ncalls, skipped = 0, set()

    def fits(what, H, L, n, nbytes):
        if nbytes <= MAX_WS_BYTES:
            return True
        skipped.add(f"{what} {H}x{L} n={n} ({nbytes / 2**30:.1f} GiB)")
        return False

    for H in WIDTHS:
        for L in DEPTHS:
            hidden = [H] * L
            cfg = hip.make_cfg(hidden)
            theta = torch.from_numpy(synth.flatten_params(synth.siren_params(hidden, seed=2))).to(dev)
            for n in SIZES:
                nh = max(1, n // 3)
                c = ctypes.byref(cfg)
                ok_q = fits("value / gradient queries, ray march", H, L, n, lib.dudf_workspace_bytes_query(c, n, 0))
                ok_h = fits("Hessian / frame queries", H, L, n, lib.dudf_workspace_bytes_query(c, n, n))
                ok_c = fits("curvature query", H, L, n, lib.dudf_workspace_bytes_curvature(c, min(n, 65536)))
                ok_t = fits("training steps, weight gradients", H, L, n, lib.dudf_workspace_bytes(c, n))
                ok_th = fits("loss_s1 step with Hessian-path points", H, L, n, lib.dudf_workspace_bytes_hess(c, n, nh))
                x, nrm, sdf = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in synth.training_batch(n, seed=3)]
                sdf = sdf.reshape(-1)
                for stash in (7, 6, 0):
                    for single in SINGLES:
                        with hip.options(stash=stash, **single):
                            if ok_q:        # queries: value, value + gradient
                                expect(cfg, n, 0, [(0, HAVE_E)], QUERY); hip.query(cfg, theta, x, want_grad=False)
                                expect(cfg, n, 0, [(0, C | HAVE_E), (1, HAVE_E)], QUERY); hip.query(cfg, theta, x)
                            if ok_h:        # Hessian, frame
                                expect(cfg, n, n, [(0, C | HAVE_E), (1, HAVE_E)], QUERY); hip.query_hessian(cfg, theta, x)
                                expect(cfg, n, n, [(0, C | HAVE_E), (1, HAVE_E)], QUERY); hip.query_frame(cfg, theta, x)
                            if ok_c:
                                expect(cfg, n, n, [(0, C | HAVE_E), (1, HAVE_E), (8, HAVE_E)], QUERY); hip.query_curvature(cfg, theta, x)
                            # loss_s1 steps without and with Hessian-path points
                            for k, w, ok in ((0, w_eik, ok_t), (nh, w_hess, ok_th)):
                                if not ok:
                                    continue
                                ws = hip.workspace_for(cfg, n, dev, n_hess=k)
                                expect(cfg, n, k, [(0, all_flags), (1, all_flags)])
                                hip.loss_forward(cfg, hip.LOSS_S1, theta, x, nrm, sdf, n, w, 100.0, ws, n_hess=k)
                                expect(cfg, n, k, [(2, TRAIN | HAVE_E), (3, TRAIN | HAVE_E)]); expect_wgrad(cfg, n, k)
                                hip.loss_backward(cfg, hip.LOSS_S1, theta, x, nrm, sdf, n, w, 100.0, ones, None, ws, n_hess=k)
                                del ws
                            if ok_t:
                                # a loss_s2 step
                                ws = hip.workspace_for(cfg, n, dev)
                                expect(cfg, n, 0, [(0, all_flags)]); st = hip.s2_forward_stats(cfg, theta, x, sdf, ws)
                                expect(cfg, n, 0, [(3, TRAIN)]); expect_wgrad(cfg, n, 0)
                                g = hip.loss_backward(cfg, hip.LOSS_S2, theta, x, nrm, sdf, n, [1e5, 1e5], 100.0, ones, st, ws)
                                # the adjoint sweeps alone, then the weight gradients by layer range
                                expect(cfg, n, 0, [(0, all_flags), (1, all_flags)])
                                hip.loss_forward(cfg, hip.LOSS_S1, theta, x, nrm, sdf, n, w_eik, 100.0, ws)
                                expect(cfg, n, 0, [(2, TRAIN | HAVE_E), (3, TRAIN | HAVE_E)])
                                hip.loss_backward_sweeps(cfg, hip.LOSS_S1, theta, nrm, sdf, n, w_eik, 100.0, ones, None, ws, n_local=n)
                                if L >= 2:
                                    expect_wgrad(cfg, n, 0); hip.weight_gradient(cfg, n, True, 1, L, g, ws)
                                hip.weight_gradient(cfg, n, True, -1, 0, g, ws)
                                del ws
                            if ok_q:        # one ray-march iteration
                                rays = torch.zeros(n, 3, dtype=torch.float64, device=dev); rays[:, 2] = 1.0
                                t0 = x.double().contiguous()
                                expect(cfg, n, 0, [(0, HAVE_E)], QUERY)
                                hip.trace_rays(cfg, theta, rays, t0, torch.ones(n, dtype=torch.uint8, device=dev), "tanh", 100.0, 1e-3, 1)
                            ncalls += 1
                torch.cuda.synchronize()
    hip.reset_options()
    json.dump(pred, open(pred_path, "w"))
    for line in sorted(skipped):
        print("left out (workspace too large):", line)
    print(f"launch census: {ncalls} call groups, {len(pred)} predicted sweep / GEMM kernels -> {pred_path}", flush=True)


def trace(directory):
    path = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))[0]
    rows = list(csv.DictReader(open(path)))
    col = lambda frag: [k for k in rows[0] if frag.lower() in k.lower()]        # noqa: E731
    name, start = col("kernel_name")[0], col("start_timestamp")[0]
    shape = sorted(col("grid_size")) + sorted(col("workgroup_size")) + sorted(col("lds"))
    rows.sort(key=lambda r: int(r[start]))
    clean = lambda s: re.sub(r"\(.*$", "", s.replace("void ", "").replace("(anonymous namespace)::", "")).replace(" ", "")   # noqa: E731
    return [(clean(r[name]),) + tuple(r[c] for c in shape) for r in rows]


def compare(dir_a, dir_b, pred_path=None):
    a, b = trace(dir_a), trace(dir_b)
    bad = sum(1 for p, q in zip(a, b) if p != q) + abs(len(a) - len(b))
    for i, (p, q) in enumerate(zip(a, b)):
        if p != q:
            print("first difference at launch", i, p, q)
            break
    print(f"kernel launches: {len(a)} and {len(b)}; differing entries: {bad}")
    if pred_path:
        pred = json.load(open(pred_path))
        seen = [r[0] for r in b if r[0].startswith("sweep_") or r[0].startswith("wgrad_hidden_")]
        wrong = sum(1 for p, q in zip(pred, seen) if p != q) + abs(len(pred) - len(seen))
        for i, (p, q) in enumerate(zip(pred, seen)):
            if p != q:
                print("first wrong prediction at", i, "predicted", p, "traced", q)
                break
        print(f"predicted sweep / GEMM kernels: {len(pred)}, traced: {len(seen)}, mismatches: {wrong}")
        bad += wrong
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(run(sys.argv[2]) if sys.argv[1] == "run" else compare(*sys.argv[2:]))
