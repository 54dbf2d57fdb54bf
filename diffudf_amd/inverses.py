# coding: utf-8
"""Distance from the hyperbolic-scaled field value — reference src/inverses.py:3-21 (numpy, host side).

Every constant is cast to a stated dtype, so the result does not hang on numpy's scalar-promotion rules: the output has the
input's floating dtype (anything else is taken as float64) and the reference's bits (tests/golden/g16_inverse.npz)."""
import numpy as np


def _floating(pred_df):
    pred_df = np.asarray(pred_df)
    return pred_df if pred_df.dtype.kind == "f" else pred_df.astype(np.float64)


def inv_tanh(pred_df, alpha, min_step=0.01):
    """t(d) = d tanh(alpha d) ~ alpha d^2 near 0: invert that branch below 1/alpha, identity above."""
    pred_df = _floating(pred_df)
    dt = pred_df.dtype.type
    return np.where(pred_df < dt(1.0 / alpha), np.sqrt(pred_df / dt(alpha)), pred_df)


def inv_squared(pred_df, alpha, min_step=0.01):
    """sqrt(f) where f > 0, else min_step; the division by sqrt(alpha) runs in float64 and is rounded back once (the
    reference's in-place `/=` by a float64 scalar)."""
    pred_df = _floating(pred_df)
    dt = pred_df.dtype.type
    out = np.full(pred_df.shape, dt(min_step), dtype=pred_df.dtype)
    pos = pred_df > 0
    out[pos] = np.sqrt(pred_df[pos])
    return (out.astype(np.float64) / np.sqrt(np.float64(alpha))).astype(pred_df.dtype)


def inv_siren(pred_df, alpha, min_step=0.01):
    pred_df = _floating(pred_df)
    return np.where(pred_df > 0, pred_df, pred_df.dtype.type(min_step))


def inverse(gt_mode, pred_df, alpha, min_step=0.01):
    table = {'siren': inv_siren, 'squared': inv_squared, 'tanh': inv_tanh}
    return table[gt_mode](pred_df, alpha, min_step)
