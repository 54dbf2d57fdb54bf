# coding: utf-8
"""Helpers of the oracle parity tests (tests/test_dtheta_edges_gpu.py, tests/test_parity_util.py): errors of d(theta) per
parameter tensor and per band of 16 rows / 16 columns of a hidden matrix (the MFMA tile edges), the seeded cases with their
fp64 oracle results (computed once per session and shared, never modified), and the launch geometry of the weight-gradient
GEMM restated from csrc/dudf_wgrad.hip.  Plain module: numpy and the oracle only, the HIP library is loaded on first use."""
import collections
import ctypes
import functools

import numpy as np

from diffudf_amd import synth
from oracle import dudf_oracle as O

W_S1EIK = [1e4, 1e4, 0.0, 1e3]
W_S1FULL = [1e4, 1e4, 1e4, 1e3]
W_S2 = [1e5, 1e5]
W_SIREN = [3e3, 1e2, 1e2, 5e1]
LOSSES = {"s1eik": ("s1", W_S1EIK), "s1full": ("s1", W_S1FULL), "s2": ("s2", W_S2), "siren": ("siren", W_SIREN)}
# the project's bars (tests/test_hip_parity.py): d(theta) and loss terms, relative to the max-norm of the reference quantity
TOL_DTHETA = {"s1eik": 1e-4, "s1full": 5e-4, "s2": 1e-4, "siren": 1e-4, "fields": 1e-4}
TOL_TERMS = {"s1eik": 1e-5, "s1full": 1e-5, "s2": 2e-5, "siren": 1e-5}
# the bar of a band of a hidden matrix: four times the worst band of the oracle run in fp32 against itself in fp64 over the small cases
# of tests/test_dtheta_edges_gpu.py (measured on the CPU, 3.53e-5 at [256]*3, 300 points, Hessian term on), at most 1e-3
BAND_FP32 = 3.53e-5
BAND_TOL = min(4 * BAND_FP32, 1e-3)


def rel(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def flat(grads):
    return np.concatenate([np.concatenate([np.asarray(w).reshape(-1), np.asarray(b).reshape(-1)]) for w, b in grads])


def tensor_slices(P):
    """[(name, begin, end, shape)] of every parameter tensor in the flat, state_dict-ordered vector of P = [(W_l, b_l)]."""
    out, o = [], 0
    for l, (w, b) in enumerate(P):
        out.append((f"dW{l}", o, o + w.size, w.shape)); o += w.size
        out.append((f"db{l}", o, o + b.size, b.shape)); o += b.size
    return out


def per_tensor_rel(got_flat, grads_ref, P):
    """[(name, max|a-b| / max|b|)] over the slice of every (W_l, b_l) of a flat d(theta) with the shapes of P."""
    got = np.asarray(got_flat, dtype=np.float64).reshape(-1)
    ref = flat(grads_ref).astype(np.float64)
    sl = tensor_slices(P)
    assert got.size == ref.size == sl[-1][2], (got.size, ref.size, sl[-1][2])
    return [(name, rel(got[a:b], ref[a:b])) for name, a, b, _ in sl]


def worst_tensor(got_flat, grads_ref, P):
    return max(per_tensor_rel(got_flat, grads_ref, P), key=lambda t: t[1])


class Band(collections.namedtuple("Band", "err axis index skipped bands")):
    """The worst band's error, 'rows' | 'cols', its index (rows / columns 16 * index ...), how many bands had a reference maximum
    of exactly zero (skipped) and how many were compared."""
    __slots__ = ()

    def __str__(self):
        return f"{self.axis} {self.index * 16}..{self.index * 16 + 15}: {self.err:.2e}"


def per_band_rel(dW_got, dW_ref, band=16):
    """max|a-b| / max|b| over every band of `band` output rows and every band of `band` input columns of one matrix (a vector:
    bands of `band` entries), each relative to that band's OWN reference maximum; returns the worst one as a `Band`.  A band
    whose reference is identically zero (padded widths only) is counted in `skipped`, not compared."""
    a = np.asarray(dW_got, dtype=np.float64); b = np.asarray(dW_ref, dtype=np.float64)
    assert a.shape == b.shape and a.ndim in (1, 2), (a.shape, b.shape)
    worst, skipped, count = (-1.0, "rows", 0), 0, 0
    for axis, name in ((0, "rows"), (1, "cols"))[:a.ndim]:
        for i, lo in enumerate(range(0, a.shape[axis], band)):
            sl = (slice(lo, lo + band),) if axis == 0 else (slice(None), slice(lo, lo + band))
            m = np.abs(b[sl]).max()
            if m == 0.0:
                skipped += 1
                continue
            count += 1
            e = np.abs(a[sl] - b[sl]).max() / m
            if not e <= worst[0]:                               # (a NaN wins)
                worst = (e, name, i)
    return Band(*worst, skipped, count)


def worst_band(got_flat, grads_ref, P):
    """(tensor name, Band) of the worst band over the hidden matrices dW1 .. dW(L-1), and the number of skipped bands."""
    got = np.asarray(got_flat).reshape(-1)
    L = len(P) - 1
    worst, skipped = None, 0
    for (name, a, b, shape), l in zip(tensor_slices(P)[2:2 * L:2], range(1, L)):
        bd = per_band_rel(got[a:b].reshape(shape), grads_ref[l][0])
        skipped += bd.skipped
        if worst is None or not bd.err <= worst[1].err:
            worst = (name, bd)
    return worst[0], worst[1], skipped


# ---- padded widths: the C ABI's layout of SIREN(3, 1, [Hp]*L) against the caller's shapes -----------------------------------------
def pad_theta(P, Hp):
    """flat theta of P zero-padded to hidden width Hp (exact for a sine MLP: hip_ops.padded_width)."""
    L = len(P) - 1
    out = []
    for l, (w, b) in enumerate(P):
        o, k = (Hp if l < L else 1), (Hp if l > 0 else 3)
        wp = np.zeros((o, k), dtype=w.dtype); wp[:w.shape[0], :w.shape[1]] = w
        bp = np.zeros(o, dtype=b.dtype); bp[:b.size] = b
        out += [wp.reshape(-1), bp]
    return np.concatenate(out)


def unpad_flat(d, P, Hp):
    """the entries of a padded flat d(theta) that belong to the caller's shapes, flat in the caller's layout"""
    L = len(P) - 1
    out, off = [], 0
    for l, (w, b) in enumerate(P):
        o, k = (Hp if l < L else 1), (Hp if l > 0 else 3)
        out.append(d[off:off + o * k].reshape(o, k)[:w.shape[0], :w.shape[1]].reshape(-1)); off += o * k
        out.append(d[off:off + o][:b.size]); off += o
    assert off == d.size
    return np.concatenate(out)


# ---- seeded cases and their oracle results -------------------------------------------------------------------------------------------
# every loss at small sizes: (hidden, n, seed), batch = thirds_batch(n, seed); the last one runs zero-padded at width 256
SMALL_NETS = [((32,) * 3, 63, 7), ((64,) * 4, 200, 11), ((128,) * 3, 130, 5), ((256, 256), 17, 3), ((256,) * 3, 300, 4),
              ((512, 512), 129, 9), ((200,) * 3, 130, 6)]
# edge column counts: (n, n_hess), batch = edge_batch(n, n_hess, seed); 4 * n_hess lands before / on / behind a 128-column pass
EDGE_NETS = [((256, 256), 21), ((512, 512), 22)]             # (hidden, seed)
EDGE_SIZES = [(1, 0), (15, 0), (16, 0), (17, 0), (127, 0), (128, 0), (129, 0), (2047, 0), (2048, 0), (2049, 0),
              (17, 17), (129, 129), (100, 1), (100, 31), (100, 32), (100, 33), (300, 100)]
# launch shapes: [256]*3 at 700 points, edge_batch(700, n_hess, LAUNCH_SEED)
LAUNCH_NET, LAUNCH_N, LAUNCH_SEED = (256,) * 3, 700, 13


def net(hidden, seed):
    """(P64, P32) of the seeded SIREN: the fp64 copy holds exactly the fp32 values the kernels read."""
    P32 = synth.siren_params(list(hidden), seed=seed, dtype=np.float32)
    return [(w.astype(np.float64), b.astype(np.float64)) for w, b in P32], P32


def thirds_batch(n, seed):
    """x, normals, sdf (n,1) fp32 of synth.training_batch: the leading third on the surface (tests/test_hip_parity.py::setup)."""
    return synth.training_batch(n, seed=seed, dtype=np.float32)


def edge_batch(n, n_hess, seed):
    """The batch of tools/stress_modes.py: rows of the seeded batch with the leading n_hess points on the surface and, when
    n_hess > 0, no other point with sdf == 0 (n_hess = 0: the batch's own leading third stays on the surface)."""
    x, nrm, sdf = synth.training_batch(max(n, 3), seed=seed + 1, dtype=np.float32)
    x, nrm, sdf = x[:n].copy(), nrm[:n].copy(), sdf[:n].copy()
    if n_hess:
        sdf[:n_hess] = 0.0
        sdf[n_hess:] = np.where(sdf[n_hess:] == 0, np.float32(0.01), sdf[n_hess:])
    return x, nrm, sdf


def s2_sdf(sdf, n_hess):
    """sdf of the loss_s2 run on an edge batch (tools/stress_modes.py): loss_s2 looks at the on-surface points only and needs two
    of them; None where the batch cannot have two."""
    n = sdf.shape[0]
    if n_hess >= 2:
        return sdf
    if n_hess == 0 and n >= 3:
        out = sdf.copy(); out[:n // 3 + 1] = 0.0
        return out
    return None


def oracle(loss, P, x, nrm, sdf, dtype=np.float64):
    """(terms (k,), grads [(dW, db)], dbg) of oracle.dudf_oracle.loss_and_grad for one of LOSSES, in `dtype`."""
    mode, w = LOSSES[loss]
    Pd = [(a.astype(dtype), b.astype(dtype)) for a, b in P]
    t, g, dbg = O.loss_and_grad(mode, Pd, x.astype(dtype), nrm.astype(dtype), sdf.astype(dtype), w, 100.0)
    return np.array([float(v) for v in t.values()]), g, dbg


@functools.lru_cache(maxsize=None)
def thirds_case(hidden, n, seed, loss):
    """fp64 oracle result of (net(hidden, seed), thirds_batch(n, seed), loss); shared by every test that asks: read only."""
    P64, _ = net(hidden, seed)
    return oracle(loss, P64, *thirds_batch(n, seed))


@functools.lru_cache(maxsize=None)
def edge_case(hidden, n, n_hess, seed, loss):
    """fp64 oracle result of (net(hidden, seed), edge_batch(n, n_hess, seed), loss) — `loss` 's2' on s2_sdf of that batch."""
    P64, _ = net(hidden, seed)
    x, nrm, sdf = edge_batch(n, n_hess, seed)
    if loss == "s2":
        sdf = s2_sdf(sdf, n_hess)
    return oracle(loss, P64, x, nrm, sdf)


def fields_oracle(P, x, ybar, gbar):
    """(y, df/dx, grads) for cotangents ybar (n,) on f and gbar (n,3) on df/dx, as tests/test_api_gpu.py::
    test_custom_loss_through_fields forms them."""
    xs = x.astype(np.float64)
    y, cache = O.forward(P, xs)
    g, rev = O.input_gradient(P, cache)
    grads, _ = O.param_grad(P, xs, cache, rev, ybar.astype(np.float64), gbar.astype(np.float64))
    return y, g, grads


def cotangents(n, seed):
    """seeded standard-normal cotangents on f (n,) and on df/dx (n,3), fp32"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n).astype(np.float32), rng.standard_normal((n, 3)).astype(np.float32)


# ---- what the weight-gradient launchers do, restated (csrc/dudf_wgrad.hip::launch_hidden, dudf_internal.h::dudf_make_layout) ---------
COL_PAD, KT = 128, 32


def wgrad_columns(n, n_hess=0):
    """columns the kernels process: four per Hessian-path point, one per other point, each range padded to 128"""
    pad = lambda c: (c + COL_PAD - 1) // COL_PAD * COL_PAD      # noqa: E731
    return max(pad(4 * n_hess) + pad(n - n_hess), COL_PAD)


def wgrad_nsplit(H, L, n, n_hess=0, cap=256, deterministic=0):
    """(nsplit, steps_total, nj): the column split of the hidden weight-gradient GEMM's grid"""
    nj, ntz = L - 1, (H // 256) ** 2 if H > 256 else 1
    steps_total = wgrad_columns(n, n_hess) // KT
    nsplit = min(cap // (nj * ntz), steps_total)
    if nsplit < 1 or deterministic:
        nsplit = 1
    return nsplit, steps_total, nj


def wgrad_kernel(cfg, n, n_hess=0):
    """name of the hidden weight-gradient kernel the library would launch under the current options (dudf_debug_kernel_choice)"""
    from diffudf_amd import _lib
    buf = ctypes.create_string_buffer(128)
    rc = _lib.load().dudf_debug_kernel_choice(ctypes.byref(cfg), int(n), int(n_hess), -1, 0, buf, len(buf))
    assert rc == 0, rc
    return buf.value.decode()
