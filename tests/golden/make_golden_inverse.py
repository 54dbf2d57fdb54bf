#!/usr/bin/env python
# coding: utf-8
"""Generate tests/golden/g16_inverse.npz by RUNNING THE REFERENCE ITSELF (same discipline as make_golden_pc.py: the reference
is resolved from its read-only mount, nothing of it is copied; build container only).

    python tests/golden/make_golden_inverse.py

The map from a field value to a step length, reference src/inverses.py:3-21 `inverse(gt_mode, pred_df, alpha, min_step)`, for
all three modes, alpha in ALPHAS (100 is the only one whose root is exact in float32), min_step in MIN_STEPS, and float32 as
well as float64 input (the reference's `evaluate` hands float64 arrays to render_mc and render_pc).

  x_{dt}_a{i}               non-negative inputs for alpha ALPHAS[i], dt in (f32, f64): 0, the smallest subnormal, 1e-30,
                            float32(1/alpha) with its two float32 neighbours [rows 3:6], 0.5, 2, and 500 seeded |N(0,1)| 2/alpha
                            (f64 only, appended: 1/alpha in float64 with its two float64 neighbours);
  y_{mode}_{dt}_a{i}_m{j}   the reference's output for them with min_step MIN_STEPS[j];
  s_a{i}                    signed float64 inputs holding float32 values (what `evaluate` returns): 0, -0.0, -0.2, 0.2, 500 seeded
                            N(0,1) 2/alpha;
  sy_{mode}_a{i}            inverse(mode, s, alpha, min_step=0) — the call of src/render_pc.py:51; 'tanh' is NaN for negatives;
  pc_samples, pc_grad       float64 positions in [-1.05, 1.05]^3 and gradients (float32 values, two zero rows), one per signed row;
  pc_moved_{mode}_a{i}, pc_accept_{mode}_a{i}   (i in PC_ALPHAS) src/render_pc.py:51-56 re-issued around the imported reference
                            `inverse` and `normalize`: samples -= steps * normalize(gradients), then the domain and threshold masks
                            with surf_thresh PC_THRESH;
  alphas, min_steps, pc_alphas, pc_thresh, numpy_version.

The archive is written with fixed member timestamps, so running the script again on the same numpy reproduces the file bit for bit.
"""
import io
import os
import sys
import zipfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, "/root/reference")          # `src.*` must resolve to the REFERENCE here, not to this repo's shim
sys.path[:] = [p for p in sys.path if os.path.abspath(p or ".") != REPO] + [REPO]

from src.inverses import inverse                                # noqa: E402  (reference)
from src.util import normalize                                  # noqa: E402  (reference)

ALPHAS = [100.0, 1.0, 3.0, 7.0, 0.5]
MIN_STEPS = [0.01, 0.0, 0.003]
MODES = ["tanh", "siren", "squared"]
PC_ALPHAS = [0, 2]                             # indices into ALPHAS
PC_THRESH = 0.01
N_RANDOM = 500


def inputs_for(alpha, rng):
    f32 = np.float32
    b = f32(1 / alpha)
    edge = np.array([0.0, np.nextafter(f32(0), f32(1)), f32(1e-30), np.nextafter(b, f32(0)), b, np.nextafter(b, f32(np.inf)),
                     0.5, 2.0], dtype=np.float32)
    draw = np.abs(rng.standard_normal(N_RANDOM)) * 2 / alpha
    x32 = np.concatenate([edge, draw.astype(np.float32)])
    b64 = 1 / alpha
    x64 = np.concatenate([edge.astype(np.float64), draw, [np.nextafter(b64, 0.0), b64, np.nextafter(b64, np.inf)]])
    return x32, x64


def write_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps and order"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    out = {"alphas": np.array(ALPHAS), "min_steps": np.array(MIN_STEPS), "pc_alphas": np.array(PC_ALPHAS, dtype=np.int64),
           "pc_thresh": np.float64(PC_THRESH), "numpy_version": np.array(np.__version__)}
    rng = np.random.default_rng(16)
    n_s = 4 + N_RANDOM
    pc_samples = rng.uniform(-1.05, 1.05, (n_s, 3))
    pc_grad = rng.standard_normal((n_s, 3)).astype(np.float32).astype(np.float64)
    pc_grad[7] = 0.0; pc_grad[0] = 0.0                          # a vanishing gradient: normalize gives NaN
    pc_samples[1] = [1.0, -1.0, 0.3]                            # on the closed domain's boundary with a zero step
    out["pc_samples"], out["pc_grad"] = pc_samples, pc_grad
    with np.errstate(invalid="ignore", divide="ignore"):
        for i, alpha in enumerate(ALPHAS):
            x32, x64 = inputs_for(alpha, rng)
            out[f"x_f32_a{i}"], out[f"x_f64_a{i}"] = x32, x64
            for mode in MODES:
                for j, ms in enumerate(MIN_STEPS):
                    for dt, x in (("f32", x32), ("f64", x64)):
                        y = inverse(mode, x.copy(), alpha, ms)
                        assert y.dtype == x.dtype and y.shape == x.shape, (mode, dt, y.dtype)
                        out[f"y_{mode}_{dt}_a{i}_m{j}"] = y
            s = np.concatenate([[0.0, -0.0, -0.2, 0.2], rng.standard_normal(N_RANDOM) * 2 / alpha])
            s = s.astype(np.float32).astype(np.float64)
            out[f"s_a{i}"] = s
            for mode in MODES:
                udfs = s.copy()[:, None]                            # (n,1), as `evaluate` returns them
                steps = inverse(mode, udfs, alpha, min_step=0)      # src/render_pc.py:51
                assert steps.dtype == np.float64
                out[f"sy_{mode}_a{i}"] = steps.flatten()
                if i in PC_ALPHAS:
                    samples = pc_samples.copy()
                    samples -= steps * normalize(pc_grad)           # :53
                    dom = np.prod(np.logical_and(samples >= -1, samples <= 1), axis=1).astype(np.bool_)     # :55
                    acc = (steps.flatten() < PC_THRESH) * dom                                                # :56
                    out[f"pc_moved_{mode}_a{i}"], out[f"pc_accept_{mode}_a{i}"] = samples, acc
    path = os.path.join(HERE, "g16_inverse.npz")
    write_npz(path, out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes,", len(out), "arrays, numpy", np.__version__)
    assert size < (512 << 10)


if __name__ == "__main__":
    main()
