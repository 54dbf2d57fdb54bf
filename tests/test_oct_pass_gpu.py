# coding: utf-8
"""GPU: the one-group ("oct") pass of the 256-wide fp16x3 sweeps against the fp64 oracle, at sizes that take seconds.

    A workgroup's share of 16-column groups is walked in passes of 8; a last pass that holds ONE group is shared by all eight
    waves (dudf_sweep_bf16.hip, sweep_tile_oct).  SIREN 3x256, plain points:
      * n = 36 864: 2304 groups over 256 workgroups, every share is 9 — EVERY workgroup ends in a one-group pass;
      * n = 32 832: 2056 groups (the columns are padded to whole 128), shares of 8 and 9 — a few workgroups end in one, the
        others run full passes only.
    Compared: y and df/dx (tolerances of tests/test_hip_parity.py) and the stash arrays s, c, q | A, e, zbar of every layer
    (tolerances of tests/test_full_size_oracle_gpu.py: 5e-5 | 2e-4), on every column of every one-group pass plus one random
    column of every 128-column pass.
    That the one-group pass is what runs is asked of the library: the kernel chosen for each of the step's four sweeps must be
    an fp16x3 build of 256-wide layers (sweep_f16*), the only ones whose driver hands a one-group pass to sweep_tile_oct.
    Points within fp32 noise of a kink of the loss are replaced as in tests/test_full_size_oracle_gpu.py (disambiguate).
"""
import ctypes

import numpy as np
import pytest
import torch

from diffudf_amd import _lib, synth
from oracle import dudf_oracle as O
from test_full_size_oracle_gpu import disambiguate

pytestmark = pytest.mark.gpu
W = [1e4, 1e4, 0.0, 1e3]
TOL_F, TOL_G = 5e-6, 2e-5


def rel(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def checked_columns(n):
    """(columns, number of one-group passes): the share arithmetic of sweep_body_b on the padded column count."""
    # mirrors launch_b (grid = min(passes of 128 columns, 256) workgroups) and sweep_body_b (workgroup b walks groups b * ng / nblk ..
    # (b + 1) * ng / nblk in passes of 8; a last pass of one group goes to sweep_tile_oct), csrc/dudf_sweep_bf16.hip: keep in step
    ng = (n + 127) // 128 * 8
    nblk = min(256, ng // 8)
    ends = [(b + 1) * ng // nblk for b in range(nblk) if ((b + 1) * ng // nblk - b * ng // nblk) % 8 == 1]
    lone = np.concatenate([16 * (g1 - 1) + np.arange(16) for g1 in ends])
    starts = np.arange(0, n, 128)
    one_per_pass = np.minimum(starts + np.random.default_rng(11).integers(0, 128, starts.size), n - 1)
    idx = np.unique(np.concatenate([lone[lone < n], one_per_pass])).astype(np.int64)
    return idx, len(ends)


@pytest.mark.parametrize("n,n_lone", [(36864, 256), (32832, 8)])
def test_one_group_pass_against_oracle(n, n_lone):
    from diffudf_amd import hip_ops as hip
    hidden = [256] * 3
    L = len(hidden)
    P32 = synth.siren_params(hidden, seed=321)
    P64 = [(w.astype(np.float64), b.astype(np.float64)) for w, b in P32]
    x, nrm, sdf = synth.training_batch(n, seed=322)
    x, nrm, sdf, n_amb = disambiguate(P64, x, nrm, sdf)
    assert n_amb < n // 100
    idx, lone = checked_columns(n)
    assert lone == n_lone
    sel = torch.from_numpy(idx).cuda()
    th = torch.from_numpy(synth.flatten_params(P32)).cuda()
    xd, nd, sd = [torch.from_numpy(a).cuda() for a in (x, nrm, sdf.reshape(-1))]
    cfg = hip.make_cfg(hidden)
    ws = hip.workspace_for(cfg, n, "cuda")
    buf = ctypes.create_string_buffer(128)                       # (sweep, flags) of a training step: tests/test_kernel_choice.py
    for which, flags in ((0, 15), (1, 15), (2, 12), (3, 12)):
        assert _lib.load().dudf_debug_kernel_choice(ctypes.byref(cfg), n, 0, which, flags, buf, len(buf)) == 0
        assert buf.value.decode().startswith("sweep_f16") and "<256," in buf.value.decode(), buf.value

    y, g = hip.fields_forward(cfg, th, xd, ws)                   # the training forward and reverse sweeps
    y, g = y[sel].double().cpu().numpy(), g[sel].double().cpu().numpy()
    y_ref, g_ref, _ = O.query(P64, x[idx].astype(np.float64))
    ef, eg = rel(y, y_ref), rel(g, g_ref)

    hip.loss_forward(cfg, hip.LOSS_S1, th, xd, nd, sd, n, W, 100.0, ws)
    hip.loss_backward(cfg, hip.LOSS_S1, th, xd, nd, sd, n, W, 100.0, torch.ones(4, device="cuda"), None, ws)
    got = {(name, l): hip.read_stash(cfg, name, l, n, ws)[sel].double().cpu().numpy()
           for name in ("s", "c", "q", "A", "e", "zbar") for l in range(L)}
    _, _, dbg = O.loss_and_grad("s1", P64, *[a[idx].astype(np.float64) for a in (x, nrm, sdf)], W, 100.0)
    f = idx.size / n                                             # the oracle's cotangents carry 1 / (its own batch size)
    worst = {}
    for l in range(L):
        for name, ref, scale in (("s", dbg["cache"]["s"][l], 1.0), ("c", dbg["cache"]["c"][l], 1.0), ("q", dbg["rev"]["q"][l], 1.0),
                                 ("A", dbg["trace"]["A"][l], f), ("e", dbg["trace"]["e"][l], f), ("zbar", dbg["trace"]["zbar"][l], f)):
            worst[name] = max(worst.get(name, 0.0), rel(got[name, l], ref * scale))
    print(f"3x256 n={n}: {lone} one-group passes, {idx.size} columns: y {ef:.2e} df/dx {eg:.2e}; stash "
          + " ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert ef < TOL_F and eg < TOL_G
    for name in ("s", "c", "q"):
        assert worst[name] < 5e-5, name
    for name in ("A", "e", "zbar"):
        assert worst[name] < 2e-4, name
