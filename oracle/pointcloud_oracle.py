# coding: utf-8
"""ORACLE — test infrastructure only.  Never imported by the product path.

numpy restatement of the projection loop of the reference's point-cloud sampler (src/render_pc.py:43-56): the samples are
float64, the network sees float32 copies and returns float32 values that `evaluate` widens to float64, and the step is
`inverse(gt_mode, udfs, alpha, min_step=0)` in float64 on the SIGNED value — no abs, so 'tanh' gives NaN for a negative one and
'siren' / 'squared' stand still.  `project_step` and `accept` are pinned by the signed block of tests/golden/g16_inverse.npz
(the same lines re-issued around the reference's `inverse` and `normalize`).
"""
import numpy as np

from . import rays_oracle as R


def project_step(samples, udfs, gradients, gt_mode, alpha):
    """One step (:51-53), in place on samples (n,3 float64).  udfs (n,), gradients (n,3): float32 values in any float dtype.
    Returns the float64 steps (n,)."""
    udfs = np.asarray(udfs, dtype=np.float64).reshape(-1)
    g = np.asarray(gradients, dtype=np.float64)
    steps = R.inverse(gt_mode, udfs, alpha, min_step=0)
    nrm = np.sqrt((g * g).sum(axis=1))
    samples -= steps[:, None] * (g / nrm[:, None])
    return steps


def accept(samples, steps, surf_thresh):
    """:55-56 — in the closed box after the move and last step below the threshold (a NaN row fails both)."""
    dom = np.logical_and(samples >= -1, samples <= 1).all(axis=1)
    return (steps < surf_thresh) & dom


def project_points(params, samples, gt_mode, alpha, num_steps=5, surf_thresh=0.01, dtype=np.float64):
    """The whole inner loop, in place on samples; returns (last steps, accept, pre-move unit gradient).  dtype: the precision
    the network itself runs in (float64: the oracle proper; float32: what the reference does)."""
    steps = unit = None
    with np.errstate(invalid="ignore", divide="ignore"):
        for _ in range(num_steps):
            udfs, g = R._query(params, samples, True, dtype=dtype)
            g64 = g.astype(np.float64)
            unit = g64 / np.sqrt((g64 * g64).sum(axis=1))[:, None]
            steps = project_step(samples, udfs, g, gt_mode, alpha)
        return steps, accept(samples, steps, surf_thresh), unit
