# coding: utf-8
"""GPU: a 12-step training trajectory of a 512-WIDE network (BASELINE configs[2]'s width) against the fp64 oracle, in its stash formats.

"The trajectory, not single-step parity, is what catches a bad format"  — and it did again in round 5: the 512-wide
kernel's relay (the stash array a layer's outputs travel through to the next layer, csrc/dudf_sweep_wide.hip::sweep_tile_w) was
built as the 24-bit fixed-point array of stash mask 7.  Every single-step tolerance held (tests/test_hip_parity.py, the full-size
oracle comparison: d(theta) 5.8e-7), config 3 ran 2.7 % faster — and THIS test, written afterwards, showed the 12-step curve leaving
the fp64 oracle's by 1.3e-5 at step 2 and 6e-4 at step 10, where the fp32 relay (masks 6 and 0) stays within 7e-7: at width 256 the
fixed-point rounding only reaches the weight-gradient GEMM's operands, in the relay it enters the layer chain itself, against a
column bound that is loose by ~w0.  The relay is fp32 again (512-wide networks get mask 6); this test stays as the bar any such
format has to pass: 12 Adam steps of the Eikonal `loss_s1` within 1e-4 of the fp64 curve (oracle/dudf_oracle.py in torch fp64 on
the CPU + its Adam), a fresh synthetic batch every step, and no format drifting more than a small factor beyond the fp32 stash."""
import numpy as np
import pytest
import torch

from diffudf_amd import synth
from oracle import dudf_oracle as O

pytestmark = pytest.mark.gpu

N, STEPS, LR = 3000, 12, 1e-4
W = [1e4, 1e4, 0.0, 1e3]


def unflatten(theta, hidden):
    dims = [3] + list(hidden) + [1]
    out, off = [], 0
    for i in range(len(dims) - 1):
        fi, fo = dims[i], dims[i + 1]
        w = theta[off:off + fo * fi].reshape(fo, fi); off += fo * fi
        b = theta[off:off + fo]; off += fo
        out.append((w, b))
    assert off == theta.size
    return out


def oracle_trajectory(HIDDEN):
    theta = synth.flatten_params(synth.siren_params(HIDDEN, seed=21)).astype(np.float64)     # the fp32 start, exactly
    m, v = np.zeros_like(theta), np.zeros_like(theta)
    hist = []
    with torch.no_grad():
        for t in range(STEPS):
            x, nrm, sdf = synth.training_batch(N, seed=9, step=t)
            Pt = [(torch.from_numpy(w.copy()), torch.from_numpy(b.copy())) for w, b in unflatten(theta, HIDDEN)]
            xs, ns, ss = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)) for a in (x, nrm, sdf)]
            terms, g, _ = O.loss_and_grad("s1", Pt, xs, ns, ss, W, 100.0, xp=torch)
            hist.append([float(val) for val in terms.values()])
            flat = torch.cat([torch.cat([w.reshape(-1), b.reshape(-1)]) for w, b in g]).numpy()
            O.adam_step(theta, flat, m, v, t + 1, LR)
    return np.array(hist)


def hip_trajectory(hip, HIDDEN):
    from diffudf_amd.engine import TrainEngine
    dev = torch.device("cuda", 0)
    theta = torch.from_numpy(synth.flatten_params(synth.siren_params(HIDDEN, seed=21))).to(dev)
    eng = TrainEngine(HIDDEN, theta)
    hist = []
    for t in range(STEPS):
        x, nrm, sdf = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in synth.training_batch(N, seed=9, step=t)]
        hist.append(eng.step(0, x, nrm, sdf.reshape(-1), W, 100.0, LR).cpu().numpy().copy())
    return np.array(hist, dtype=np.float64)


@pytest.mark.parametrize("width", [512, 256])
def test_12_steps_against_the_fp64_oracle_in_every_stash_format(width):
    """width 512: masks 6 (what a 512-wide workspace gets when 7 is asked for) and 0; width 256, the same protocol for comparison:
    masks 7 (default: the fixed-point arrays feed only the weight-gradient GEMM there), 6 and 0."""
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible")
    from diffudf_amd import hip_ops as hip
    hidden = [width] * 8
    ref = oracle_trajectory(hidden)
    assert np.isfinite(ref).all() and (ref[:, 2] == 0).all()
    worst = {}
    for stash in (7, 6, 0):
        with hip.options(stash=stash):
            mode = hip.stash_mode(hip.make_cfg(hidden), N)
            assert mode == (6 if (stash == 7 and width == 512) else stash)
            if mode in worst:
                continue
            got = hip_trajectory(hip, hidden)
        err = np.abs(got - ref).max(axis=1) / np.abs(ref).max(axis=1)
        worst[mode] = float(err.max())
        print(f"8x{width}, {N} points, stash mask {mode}: per-step error against the fp64 oracle {np.array2string(err, precision=1)}")
    for mode, wv in worst.items():
        assert wv < 1e-4, (mode, worst)                  # the north star's bar
        assert wv < 1e-5, (mode, worst)                  # ... and what the build holds (measured: 7e-7 at width 512)
    # no format drifts far beyond the fp32 stash: they all leave the fp64 curve at the rate fp32 arithmetic does
    for mode in worst:
        assert worst[mode] < 10.0 * worst[0] + 2e-6, worst
