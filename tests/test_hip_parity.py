# coding: utf-8
"""GPU parity: the HIP path (through the C ABI) against the oracle on the same seeded inputs.

Tolerances (relative to the max-norm of the reference quantity) follow the fp32 noise floor of the
reference itself against its own fp64 run (re-measured in
tests/test_oracle_golden.py::test_g2_8x256_fields_and_grads):
    value 5e-6, df/dx 2e-5, loss terms 1e-5, parameter gradient 1e-4 (Eikonal path).
"""
import os
import numpy as np
import pytest
import torch

from diffudf_amd import synth
from oracle import dudf_oracle as O

pytestmark = pytest.mark.gpu

TOL_F, TOL_G, TOL_TERM, TOL_DTHETA = 5e-6, 2e-5, 1e-5, 1e-4
W_S1EIK = [1e4, 1e4, 0.0, 1e3]
W_S2 = [1e5, 1e5]
W_SIREN = [3e3, 1e2, 1e2, 5e1]


def rel(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def flat(grads):
    return np.concatenate([np.concatenate([w.reshape(-1), b.reshape(-1)]) for w, b in grads])


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible")
    from diffudf_amd import hip_ops
    return hip_ops


def setup(hidden, n, seed):
    P32 = synth.siren_params(hidden, seed=seed, dtype=np.float32)
    theta = synth.flatten_params(P32)
    x, nrm, sdf = synth.training_batch(n, seed=seed, dtype=np.float32)
    P64 = [(w.astype(np.float64), b.astype(np.float64)) for w, b in P32]
    return P64, theta, x, nrm, sdf


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# [256, 256] and [256]*3: the shortest chunk streams the bf16x6 kernel sees (one / two hidden matrices), with column counts
# that leave idle waves (17 columns) and a partial last pass (129)
NETS = [([32, 32, 32], 63, 7), ([64] * 4, 200, 11), ([128] * 3, 130, 5), ([256] * 8, 1000, 123),
        ([256, 256], 17, 3), ([256] * 3, 129, 4)]
NETS_WIDE = NETS + [([512] * 3, 300, 9)]          # BASELINE configs[2]'s width (8x512 is exercised by bench.py --hidden 512)


@pytest.mark.parametrize("hidden,n,seed", NETS_WIDE)
def test_query_value_and_gradient(hip, hidden, n, seed):
    P, theta, x, _, _ = setup(hidden, n, seed)
    cfg = hip.make_cfg(hidden)
    f, g = hip.query(cfg, dev(theta), dev(x), want_grad=True)
    y_ref, g_ref, _ = O.query(P, x.astype(np.float64))
    ef, eg = rel(f.cpu().numpy(), y_ref), rel(g.cpu().numpy(), g_ref)
    print(f"query {hidden[0]}x{len(hidden)} n={n}: f {ef:.2e} g {eg:.2e}")
    assert ef < TOL_F and eg < TOL_G
    f2, g2 = hip.query(cfg, dev(theta), dev(x), want_grad=False)
    assert g2 is None and rel(f2.cpu().numpy(), y_ref) < TOL_F


@pytest.mark.parametrize("hidden,n,seed", NETS_WIDE)
@pytest.mark.parametrize("case,mode,w", [("s1eik", "s1", W_S1EIK), ("siren", "siren", W_SIREN)])
def test_loss_and_parameter_gradient(hip, hidden, n, seed, case, mode, w):
    P, theta, x, nrm, sdf = setup(hidden, n, seed)
    cfg = hip.make_cfg(hidden)
    ws = hip.workspace_for(cfg, n, "cuda")
    m = {"s1": hip.LOSS_S1, "siren": hip.LOSS_SIREN}[mode]
    th, xd, nd, sd = dev(theta), dev(x), dev(nrm), dev(sdf.reshape(-1))
    terms = hip.loss_forward(cfg, m, th, xd, nd, sd, n, w, 100.0, ws)
    t_ref, g_ref, dbg = O.loss_and_grad(mode, P, x.astype(np.float64), nrm.astype(np.float64), sdf.astype(np.float64), w, 100.0)
    t_ref = np.array([float(v) for v in t_ref.values()])
    # stage-by-stage: what the forward sweeps stashed
    L = len(hidden)
    for l in range(L):
        for name, ref in (("s", dbg["cache"]["s"][l]), ("c", dbg["cache"]["c"][l]), ("q", dbg["rev"]["q"][l])):
            got = hip.read_stash(cfg, name, l, n, ws).cpu().numpy()
            e = rel(got, ref)
            assert e < 5e-5, f"{case} stash {name}[{l}] rel err {e:.2e}"
    et = rel(terms.cpu().numpy(), t_ref)
    cot = torch.ones(4, device="cuda")
    dth = hip.loss_backward(cfg, m, th, xd, nd, sd, n, w, 100.0, cot, None, ws)
    for l in range(L):
        for name, ref in (("A", dbg["trace"]["A"][l]), ("e", dbg["trace"]["e"][l]), ("zbar", dbg["trace"]["zbar"][l])):
            got = hip.read_stash(cfg, name, l, n, ws).cpu().numpy()
            e = rel(got, ref)
            assert e < 2e-4, f"{case} stash {name}[{l}] rel err {e:.2e}"
    ed = rel(dth.cpu().numpy(), flat(g_ref))
    print(f"{case} {hidden[0]}x{L} n={n}: terms {et:.2e} dtheta {ed:.2e}")
    assert et < TOL_TERM
    assert ed < TOL_DTHETA
    # cotangent scaling: backward is linear in cot
    cot2 = torch.tensor([0.5, 2.0, 3.0, 0.25], device="cuda")
    t2, g2, _ = O.loss_and_grad(mode, P, x.astype(np.float64), nrm.astype(np.float64), sdf.astype(np.float64),
                                [w[i] * float(cot2[i]) for i in range(4)], 100.0)
    dth2 = hip.loss_backward(cfg, m, th, xd, nd, sd, n, w, 100.0, cot2, None, ws)
    assert rel(dth2.cpu().numpy(), flat(g2)) < TOL_DTHETA


@pytest.mark.parametrize("hidden,n,seed", NETS_WIDE)
def test_loss_s2(hip, hidden, n, seed):
    P, theta, x, nrm, sdf = setup(hidden, n, seed)
    cfg = hip.make_cfg(hidden)
    ws = hip.workspace_for(cfg, n, "cuda")
    th, xd, nd, sd = dev(theta), dev(x), dev(nrm), dev(sdf.reshape(-1))
    stats = hip.s2_forward_stats(cfg, th, xd, sd, ws)
    terms = hip.s2_terms(stats, W_S2)
    t_ref, g_ref, _ = O.loss_and_grad("s2", P, x.astype(np.float64), nrm.astype(np.float64), sdf.astype(np.float64), W_S2, 100.0)
    t_ref = np.array([float(v) for v in t_ref.values()])
    cot = torch.ones(4, device="cuda")
    dth = hip.loss_backward(cfg, hip.LOSS_S2, th, xd, nd, sd, n, W_S2, 100.0, cot, stats, ws)
    et, ed = rel(terms.cpu().numpy(), t_ref), rel(dth.cpu().numpy(), flat(g_ref))
    print(f"s2 {hidden[0]}x{len(hidden)} n={n}: terms {et:.2e} dtheta {ed:.2e}")
    assert et < 2e-5 and ed < TOL_DTHETA


TOL_H = 2e-5
W_S1FULL = [1e4, 1e4, 1e4, 1e3]


@pytest.mark.parametrize("hidden,n,seed", NETS_WIDE)
def test_query_hessian(hip, hidden, n, seed):
    P, theta, x, _, _ = setup(hidden, n, seed)
    cfg = hip.make_cfg(hidden)
    f, g, h = hip.query_hessian(cfg, dev(theta), dev(x))
    xs = x.astype(np.float64)
    y_ref, g_ref, H_ref = O.query(P, xs, want_grad=True, want_hess=True)
    ef, eg, eh = rel(f.cpu().numpy(), y_ref), rel(g.cpu().numpy(), g_ref), rel(h.cpu().numpy(), H_ref)
    print(f"hessian {hidden[0]}x{len(hidden)} n={n}: f {ef:.2e} g {eg:.2e} H {eh:.2e}")
    assert ef < TOL_F and eg < TOL_G and eh < TOL_H


@pytest.mark.parametrize("hidden,n,seed", NETS_WIDE)
def test_loss_s1_with_hessian_term(hip, hidden, n, seed):
    """The full reference training loss (configs/train_cfg.json weights): Hessian + eigh + its backward."""
    P, theta, x, nrm, sdf = setup(hidden, n, seed)
    n_on = int((sdf[:, 0] == 0).sum())
    assert (sdf[:n_on, 0] == 0).all() and n_on == n // 3
    cfg = hip.make_cfg(hidden)
    ws = hip.workspace_for(cfg, n, "cuda", n_hess=n_on)
    th, xd, nd, sd = dev(theta), dev(x), dev(nrm), dev(sdf.reshape(-1))
    terms = hip.loss_forward(cfg, hip.LOSS_S1, th, xd, nd, sd, n, W_S1FULL, 100.0, ws, n_hess=n_on)
    t_ref, g_ref, dbg = O.loss_and_grad("s1", P, x.astype(np.float64), nrm.astype(np.float64), sdf.astype(np.float64),
                                        W_S1FULL, 100.0)
    t_ref = np.array([float(v) for v in t_ref.values()])
    et = rel(terms.cpu().numpy(), t_ref)
    dth = hip.loss_backward(cfg, hip.LOSS_S1, th, xd, nd, sd, n, W_S1FULL, 100.0, torch.ones(4, device="cuda"), None,
                            ws, n_hess=n_on)
    ed = rel(dth.cpu().numpy(), flat(g_ref))
    print(f"s1full {hidden[0]}x{len(hidden)} n={n}: terms {et:.2e} dtheta {ed:.2e}")
    assert et < TOL_TERM
    assert ed < 5e-4            # the reference's own fp32 noise with the Hessian term on is 6e-5


def test_against_committed_reference_fixture(hip, golden_dir):
    """HIP vs the reference's own fp32 outputs (golden fixture), not just vs the oracle."""
    G = np.load(os.path.join(golden_dir, "g2_8x256.npz"))
    hidden = list(G["hidden"]); n = int(G["n_points"])
    P, theta, x, nrm, sdf = setup(hidden, n, int(G["param_seed"]))
    cfg = hip.make_cfg(hidden)
    ws = hip.workspace_for(cfg, n, "cuda")
    th, xd, nd, sd = dev(theta), dev(x), dev(nrm), dev(sdf.reshape(-1))
    f, g = hip.query(cfg, th, xd)
    assert rel(f.cpu().numpy(), G["f64_y"]) < TOL_F
    assert rel(g.cpu().numpy(), G["f64_g"]) < TOL_G
    terms = hip.loss_forward(cfg, hip.LOSS_S1, th, xd, nd, sd, n, W_S1EIK, 100.0, ws)
    assert rel(terms.cpu().numpy(), G["f64_s1eik_terms"]) < TOL_TERM
    dth = hip.loss_backward(cfg, hip.LOSS_S1, th, xd, nd, sd, n, W_S1EIK, 100.0, torch.ones(4, device="cuda"), None, ws)
    d = dth.cpu().numpy()
    assert rel(d[G["sample"]], G["f64_s1eik_dtheta_sample"]) < TOL_DTHETA
    assert abs(np.linalg.norm(d.astype(np.float64)) - G["f64_s1eik_dtheta_norm"][0]) / G["f64_s1eik_dtheta_norm"][0] < 1e-5


def test_adam_step_matches_torch_semantics(hip):
    rng = np.random.default_rng(0)
    n = 10007
    theta = rng.standard_normal(n).astype(np.float32); g = rng.standard_normal(n).astype(np.float32) * 1e-2
    th = dev(theta.copy()); m = torch.zeros(n, device="cuda"); v = torch.zeros(n, device="cuda")
    ref = theta.astype(np.float64).copy(); mr = np.zeros(n); vr = np.zeros(n)
    for t in range(1, 6):
        gg = g * t
        hip.adam_step(th, dev(gg), m, v, t, 1e-3)
        O.adam_step(ref, gg.astype(np.float64), mr, vr, t, 1e-3)
    assert rel(th.cpu().numpy(), ref) < 1e-6


def test_adam_step_tracks_torch_optim_adam(hip):
    """dudf_adam_step against torch.optim.Adam ON THE GPU (what the reference loop runs, train.py:334-337): the same
    operations with the same constants, so after 12 steps theta differs by rounding-order effects only (a 1 - beta2
    formed in float would show up here as 1e-5)."""
    rng = np.random.default_rng(3)
    n = 40013
    theta = (rng.standard_normal(n) * 5e-3).astype(np.float32)
    p = torch.nn.Parameter(dev(theta.copy()))
    opt = torch.optim.Adam([p], lr=1e-4)
    th = dev(theta.copy()); m = torch.zeros(n, device="cuda"); v = torch.zeros(n, device="cuda")
    for t in range(1, 13):
        g = dev((rng.standard_normal(n) * 10.0 ** rng.uniform(-2, 2, n)).astype(np.float32))
        p.grad = g.clone()
        opt.step()
        hip.adam_step(th, g, m, v, t, 1e-4)
    a, b = th.cpu().numpy().astype(np.float64), p.detach().cpu().numpy().astype(np.float64)
    st = opt.state[p]
    em = rel(m.cpu().numpy(), st["exp_avg"].cpu().numpy()); ev = rel(v.cpu().numpy(), st["exp_avg_sq"].cpu().numpy())
    print(f"adam vs torch.optim.Adam after 12 steps: theta {rel(a, b):.2e} (identical: {np.array_equal(a, b)}), "
          f"exp_avg {em:.2e}, exp_avg_sq {ev:.2e}")
    assert rel(a, b) < 2e-7 and em < 5e-7 and ev < 5e-7
    # in units of the update itself (12 steps of ~lr each): well under a percent of one step
    assert np.abs(a - b).max() < 1e-2 * 1e-4


def test_unsupported_configs_fail_loudly(hip):
    from diffudf_amd import _lib
    cfg = hip.make_cfg([64] * 2)
    ws = hip.workspace_for(cfg, 128, "cuda")
    z = torch.zeros(128, 3, device="cuda")
    th = torch.zeros(hip.theta_count(cfg), device="cuda")
    with pytest.raises(_lib.DudfError):      # a Hessian range with a loss that has no Hessian term
        hip.loss_forward(cfg, hip.LOSS_SIREN, th, z, z, z[:, 0].contiguous(), 128, [1, 1, 1, 1], 100.0, ws, n_hess=4)
    # any list of widths runs at the smallest built width >= its widest layer (round 3; tests/test_api_gpu.py::
    # test_any_hidden_layer_config) ...
    assert hip.make_cfg([64, 32]).hidden == 64 and hip.make_cfg([48, 48]).hidden == 64 and hip.make_cfg([300, 20]).hidden == 512
    with pytest.raises(_lib.DudfError):      # ... but theta must have that network's (padded) size,
        hip.query(hip.make_cfg([48, 48, 48]), th, z)
    with pytest.raises(_lib.DudfError):      # widths beyond the built set,
        hip.make_cfg([1024] * 2)
    with pytest.raises(_lib.DudfError):      # empty / non-positive widths
        hip.make_cfg([64, 0])
    with pytest.raises(_lib.DudfError):      # and anything but 3-D points -> scalar field still have no HIP path
        hip.make_cfg([64, 64], n_in=2)


def test_f32_and_bf16x6_sweeps_agree(hip):
    """The 256-wide plain path runs its hidden matmuls on the 16-bit matrix cores — fp16 hi/lo split, three products
    (default since round 3) or the exact 3-way bf16 split, six products (option split = 0; csrc/dudf_sweep_bf16.hip, csrc/dudf_sweep16.h) —;
    options sweep_family = 0 / wgrad_family = 1 select the f32-input MFMA kernels.  All three must meet the SAME oracle
    tolerances, and agree with each other far inside them.  The modes are switched IN-PROCESS through dudf_set_option
    (rounds 1-4 read environment variables once per process and needed a child process per mode)."""
    hid = [256] * 8
    th = torch.from_numpy(synth.flatten_params(synth.siren_params(hid, seed=123))).cuda()
    xd, nd, sd = [torch.from_numpy(a).cuda() for a in synth.training_batch(1000, seed=5, step=0)]
    cfg = hip.make_cfg(hid)
    w = [1e4, 1e4, 0.0, 1e3]

    def run():
        ws = hip.workspace_for(cfg, 1000, th.device)
        terms = hip.loss_forward(cfg, 0, th, xd, nd, sd, 1000, w, 100.0, ws)
        g = hip.loss_backward(cfg, 0, th, xd, nd, sd, 1000, w, 100.0, torch.ones(4, device="cuda"), None, ws)
        f, gr = hip.query(cfg, th, xd)
        return dict(terms=terms.cpu().numpy(), g=g.cpu().numpy(), f=f.cpu().numpy(), gr=gr.cpu().numpy())
    outs = {}
    for tag, opts in (("fp16", {}), ("bf16", {"split": 0}), ("f32", {"sweep_family": 0, "wgrad_family": 1})):
        with hip.options(**opts):
            outs[tag] = run()
    P = synth.siren_params([256] * 8, seed=123, dtype=np.float64)
    x, nrm, sdf = synth.training_batch(1000, seed=5, step=0)
    terms, grads, dbg = O.loss_and_grad("s1", P, x.astype(np.float64), nrm.astype(np.float64), sdf.astype(np.float64),
                                        [1e4, 1e4, 0.0, 1e3], 100.0)
    gref = np.concatenate([np.concatenate([w.reshape(-1), b.reshape(-1)]) for w, b in grads])
    for tag in ("fp16", "bf16", "f32"):
        assert rel(outs[tag]["f"], dbg["y"]) < 5e-6, tag
        assert rel(outs[tag]["gr"], dbg["g"]) < 2e-5, tag
        assert rel(outs[tag]["g"], gref) < 1e-4, tag
        assert rel(outs[tag]["terms"], np.array(list(terms.values()))) < 1e-5, tag
    assert rel(outs["bf16"]["f"], outs["f32"]["f"]) < 2e-6
    assert rel(outs["bf16"]["g"], outs["f32"]["g"]) < 5e-6
    assert rel(outs["fp16"]["f"], outs["f32"]["f"]) < 2.5e-6          # fp16x3 vs f32: the same bars (+ the 2^-23 worst-case piece)
    assert rel(outs["fp16"]["gr"], outs["f32"]["gr"]) < 5e-6
    assert rel(outs["fp16"]["g"], outs["f32"]["g"]) < 5e-6
    assert rel(outs["fp16"]["g"], outs["bf16"]["g"]) < 5e-6


@pytest.mark.parametrize("scale", [1e-12, 1e-4, 1.0, 1e6, 1e12, 2.0 ** -40, 2.0 ** 40])
def test_fp16x3_range_scaling(hip, scale):
    """fp16x3 buys fp16's range with powers of two: per matrix (weights), per column (the sweeps' B operands), per layer
    (the weight-gradient GEMM's operands).  The backward is linear in the upstream cotangent, so scaling `cot` by 1e-12 ...
    1e12 moves every adjoint quantity (A_l, e_l, zbar_l) across 24 decades — far outside fp16 — and d(theta) must simply
    scale with it; a network whose hidden weights are 4x larger / 64x smaller than SIREN's init exercises the weight scale
    (much larger weights push the sine arguments to hundreds of radians, where fp32 itself — the reference's too — is off)."""
    hidden, n = [256] * 4, 700
    P, theta, x, nrm, sdf = setup(hidden, n, 21)
    cfg = hip.make_cfg(hidden)
    ws = hip.workspace_for(cfg, n, "cuda")
    th, xd, nd, sd = dev(theta), dev(x), dev(nrm), dev(sdf.reshape(-1))
    hip.loss_forward(cfg, hip.LOSS_S1, th, xd, nd, sd, n, W_S1EIK, 100.0, ws)
    g1 = hip.loss_backward(cfg, hip.LOSS_S1, th, xd, nd, sd, n, W_S1EIK, 100.0, torch.ones(4, device="cuda"), None, ws).clone()
    gs = hip.loss_backward(cfg, hip.LOSS_S1, th, xd, nd, sd, n, W_S1EIK, 100.0, torch.full((4,), scale, device="cuda"), None, ws)
    assert torch.isfinite(gs).all()
    # 2e-6: fp32's own noise at 700 points — held by the default stash (R, E, C at 24 bits: measured 3.5e-7 with R, E alone).  With the opt-in
    # all-24-bit stash (dudf_stash_mode 7) a cotangent scaled by a NON-power of two rounds the weight-gradient GEMM's operands at
    # other places — 2^-17 = 7.6e-6 per element, the format's bound, is then the bar for this self-consistency check (measured
    # 2.0e-6); powers of two commute with the rounding and keep the fp32 bar.
    pow2 = float(np.log2(scale)).is_integer()
    lin = rel((gs.double() / scale).cpu().numpy(), g1.double().cpu().numpy())
    print(f"linearity in the cotangent, scale {scale:g}, stash mode {hip.stash_mode(cfg, n)}: {lin:.2e}")
    assert lin < (2e-6 if pow2 or hip.stash_mode(cfg, n) != 7 else 8e-6), scale
    if scale in (1e-4, 1e6):                             # weights far from the init's size: oracle-direct
        k = 4.0 if scale > 1 else 1.0 / 64.0
        P2 = [(w * (k if 0 < i < len(P) - 1 else 1.0), b) for i, (w, b) in enumerate(P)]
        th2 = dev(np.concatenate([np.concatenate([w.reshape(-1), b.reshape(-1)]) for w, b in P2]).astype(np.float32))
        P2 = [(w.astype(np.float32).astype(np.float64), b) for w, b in P2]
        terms = hip.loss_forward(cfg, hip.LOSS_S1, th2, xd, nd, sd, n, W_S1EIK, 100.0, ws)
        g2 = hip.loss_backward(cfg, hip.LOSS_S1, th2, xd, nd, sd, n, W_S1EIK, 100.0, torch.ones(4, device="cuda"), None, ws)
        t_ref, g_ref, _ = O.loss_and_grad("s1", P2, x.astype(np.float64), nrm.astype(np.float64), sdf.astype(np.float64), W_S1EIK, 100.0)
        assert rel(terms.cpu().numpy(), np.array([float(v) for v in t_ref.values()])) < 1e-5, k
        assert rel(g2.cpu().numpy(), flat(g_ref)) < (1e-4 if k < 1 else 3e-4), k


@pytest.mark.parametrize("scale", [1e-10, 1e8])
def test_fp16x3_range_scaling_hessian_quads(hip, scale):
    """The same for the Hessian quads (fp16x3 since round 3: csrc/dudf_sweep_bf16.hip, `set_scale`): their tails couple the four
    channels of a quad, so a column's power of two comes from a bound over its own and its quad's accumulators, max_f |zdot_l|
    (left by the quads' forward sweep) and max_f |e_l|.  Linear in the upstream cotangent over 18 decades; a network with 4x
    larger hidden weights (tangent channels ~4^L larger) against the oracle."""
    hidden, n = [256] * 4, 600
    P, theta, x, nrm, sdf = setup(hidden, n, 23)
    n_on = n // 3
    cfg = hip.make_cfg(hidden)
    ws = hip.workspace_for(cfg, n, "cuda", n_hess=n_on)
    th, xd, nd, sd = dev(theta), dev(x), dev(nrm), dev(sdf.reshape(-1))
    hip.loss_forward(cfg, hip.LOSS_S1, th, xd, nd, sd, n, W_S1FULL, 100.0, ws, n_hess=n_on)
    g1 = hip.loss_backward(cfg, hip.LOSS_S1, th, xd, nd, sd, n, W_S1FULL, 100.0, torch.ones(4, device="cuda"), None, ws, n_hess=n_on).clone()
    gs = hip.loss_backward(cfg, hip.LOSS_S1, th, xd, nd, sd, n, W_S1FULL, 100.0, torch.full((4,), scale, device="cuda"), None, ws, n_hess=n_on)
    assert torch.isfinite(gs).all()
    # (opt-in all-24-bit stash: a cotangent scaled by a non-power of two rounds the stashed operands at other places — the format's
    #  own 2^-17 per element bounds this self-consistency check there, see test_fp16x3_range_scaling; measured 8.0e-6.  Default
    #  stash, R, E (and C) at 24 bits: 1.6e-6)
    lin = rel((gs.double() / scale).cpu().numpy(), g1.double().cpu().numpy())
    print(f"linearity in the cotangent (quads), scale {scale:g}, stash mode {hip.stash_mode(cfg, n)}: {lin:.2e}")
    assert lin < (5e-6 if hip.stash_mode(cfg) != 7 else 2e-5), scale
    if scale > 1:
        k = 4.0
        P2 = [(w * (k if 0 < i < len(P) - 1 else 1.0), b) for i, (w, b) in enumerate(P)]
        th2 = dev(np.concatenate([np.concatenate([w.reshape(-1), b.reshape(-1)]) for w, b in P2]).astype(np.float32))
        P2 = [(w.astype(np.float32).astype(np.float64), b) for w, b in P2]
        terms = hip.loss_forward(cfg, hip.LOSS_S1, th2, xd, nd, sd, n, W_S1FULL, 100.0, ws, n_hess=n_on)
        g2 = hip.loss_backward(cfg, hip.LOSS_S1, th2, xd, nd, sd, n, W_S1FULL, 100.0, torch.ones(4, device="cuda"), None, ws, n_hess=n_on)
        t_ref, g_ref, _ = O.loss_and_grad("s1", P2, x.astype(np.float64), nrm.astype(np.float64), sdf.astype(np.float64), W_S1FULL, 100.0)
        assert rel(terms.cpu().numpy(), np.array([float(v) for v in t_ref.values()])) < 2e-5, k
        assert rel(g2.cpu().numpy(), flat(g_ref)) < 2e-3, k          # sine arguments of hundreds of radians: fp32's own floor


def test_deterministic_mode_is_bit_reproducible(hip):
    """Option deterministic = 1 (SURVEY.md §5 'race detection' row): every cross-workgroup sum has one owner, so loss terms,
    loss_s2 statistics and d(theta) are BIT-IDENTICAL across launches — for the Eikonal loss, the Hessian loss (quad
    columns) and stage 2, at a batch that spans several workgroup passes, and for a two-shard accumulation.  The
    default build sums partial tiles with float atomics: its launches agree to rounding only (checked too, so that the
    test would notice if the switch stopped doing anything).  What cannot be bit-identical in fp32 is 1-vs-N shards: the
    shards' partial sums are rounded before they are added (they agree to ~1e-7, tests/test_multirank_gpu.py)."""
    hid = [256] * 8
    n = 5000
    th = torch.from_numpy(synth.flatten_params(synth.siren_params(hid, seed=123))).cuda()
    x, nrm, sdf = [torch.from_numpy(a).cuda() for a in synth.training_batch(n, seed=9, step=0)]
    sdf = sdf.reshape(-1)
    cfg = hip.make_cfg(hid)
    ones = torch.ones(4, device="cuda")

    def run():
        out = {}
        for rep in range(3):
            ws = hip.workspace_for(cfg, n, th.device)
            t = hip.loss_forward(cfg, 0, th, x, nrm, sdf, n, [1e4, 1e4, 0.0, 1e3], 100.0, ws)
            g = hip.loss_backward(cfg, 0, th, x, nrm, sdf, n, [1e4, 1e4, 0.0, 1e3], 100.0, ones, None, ws)
            out["eik_t%d" % rep] = t.cpu().numpy(); out["eik_g%d" % rep] = g.cpu().numpy()
            nh = int((sdf == 0).sum())
            wsh = hip.workspace_for(cfg, n, th.device, n_hess=nh)
            t = hip.loss_forward(cfg, 0, th, x, nrm, sdf, n, [1e4, 1e4, 1e4, 1e3], 100.0, wsh, n_hess=nh)
            g = hip.loss_backward(cfg, 0, th, x, nrm, sdf, n, [1e4, 1e4, 1e4, 1e3], 100.0, ones, None, wsh, n_hess=nh)
            out["full_t%d" % rep] = t.cpu().numpy(); out["full_g%d" % rep] = g.cpu().numpy()
            ws = hip.workspace_for(cfg, n, th.device)
            st = hip.s2_forward_stats(cfg, th, x, sdf, ws)
            g = hip.loss_backward(cfg, 1, th, x, nrm, sdf, n, [1e5, 1e5], 100.0, ones, st, ws)
            out["s2_t%d" % rep] = st.cpu().numpy(); out["s2_g%d" % rep] = g.cpu().numpy()
            # two uneven shards of the same batch accumulated into one d(theta) (accumulate = 1), in a fixed order
            acc = torch.zeros_like(th)
            for a, b in ((0, 1777), (1777, n)):
                xs, ns, ss = x[a:b].contiguous(), nrm[a:b].contiguous(), sdf[a:b].contiguous()
                w2 = hip.workspace_for(cfg, b - a, th.device)
                hip.loss_forward(cfg, 0, th, xs, ns, ss, n, [1e4, 1e4, 0.0, 1e3], 100.0, w2)
                hip.loss_backward(cfg, 0, th, xs, ns, ss, n, [1e4, 1e4, 0.0, 1e3], 100.0, ones, None, w2, dtheta=acc, accumulate=True)
            out["shard_g%d" % rep] = acc.cpu().numpy()
        return out
    res = {}
    for tag, opts in (("det", {"deterministic": 1}), ("atomic", {})):
        with hip.options(**opts):
            res[tag] = run()
    d, a = res["det"], res["atomic"]
    for k in ("eik_t", "eik_g", "full_t", "full_g", "s2_t", "s2_g", "shard_g"):
        assert np.array_equal(d[k + "0"], d[k + "1"]) and np.array_equal(d[k + "0"], d[k + "2"]), k   # bit for bit
        assert rel(a[k + "0"], d[k + "0"]) < (5e-5 if k.startswith("full") else 2e-6), k              # same numbers
    assert rel(d["shard_g0"], d["eik_g0"]) < 2e-6                 # shards: equal to rounding, not to the bit
    moved = sum(not np.array_equal(a[k + "0"], a[k + "1"]) for k in ("eik_g", "full_g", "s2_g", "shard_g"))
    print("deterministic mode: all bit-identical; default mode: %d of 4 gradients differ in the last bits between launches" % moved)


@pytest.mark.parametrize("mode,w", [(0, W_S1EIK), (1, W_S2)])
def test_weight_gradient_by_layer_ranges(hip, mode, w):
    """dudf_loss_backward_sweeps + dudf_weight_gradient over layer groups (what the multi-GPU step overlaps with its
    all-reduces) reproduces dudf_loss_backward: every slice of d(theta) is written by exactly one call."""
    hidden, n, seed = [256] * 8, 1000, 123
    P, theta, x, nrm, sdf = setup(hidden, n, seed)
    cfg = hip.make_cfg(hidden)
    ws = hip.workspace_for(cfg, n, "cuda")
    th, xd, nd, sd = dev(theta), dev(x), dev(nrm), dev(sdf.reshape(-1))
    ones = torch.ones(4, device="cuda")

    def forward():
        if mode == 1:
            return hip.s2_forward_stats(cfg, th, xd, sd, ws)
        hip.loss_forward(cfg, mode, th, xd, nd, sd, n, w, 100.0, ws)
        return None
    stats = forward()
    ref = hip.loss_backward(cfg, mode, th, xd, nd, sd, n, w, 100.0, ones, stats, ws).clone()
    stats = forward()
    got = torch.full_like(ref, float("nan"))                     # every element must be overwritten
    hip.loss_backward_sweeps(cfg, mode, th, nd, sd, n, w, 100.0, ones, stats, ws, n_local=n)
    L = len(hidden)
    for b, e in ((6, 8), (3, 6), (1, 3)):
        hip.weight_gradient(cfg, n, mode != 1, b, e, got, ws)
    hip.weight_gradient(cfg, n, mode != 1, -1, 0, got, ws)
    assert torch.isfinite(got).all()
    assert rel(got.cpu().numpy(), ref.cpu().numpy()) < 2e-6
    sl = hip.layer_slices(cfg)
    assert sl[0] == (0, 4 * 256) and sl[L][1] == ref.numel() and all(sl[i][1] == sl[i + 1][0] for i in range(L))


def test_pair_launch_agrees_with_separate_launches(hip):
    """A training batch with Hessian-path points runs every sweep as ONE grid for its quad columns and its plain
    columns (csrc/dudf_sweep_bf16.hip: sweep_pair_kernel; the host splits the 256 workgroups between the two);
    option pair_launch = 0 launches them one after the other.  Same numbers either way — at a size where both parts take several
    passes per workgroup and the split is uneven (40 000 points, 13 333 on the Hessian path) and at one where the pair has
    fewer tiles than CUs — and both meet the oracle on a subset of the points."""
    hid = [256] * 4
    th = torch.from_numpy(synth.flatten_params(synth.siren_params(hid, seed=31))).cuda()
    cfg = hip.make_cfg(hid)

    def run():
        out = {}
        for n in (40000, 900):
            nh = n // 3                                  # the leading on-surface third (synth.training_batch)
            x, nrm, sdf = [torch.from_numpy(a).cuda() for a in synth.training_batch(n, seed=6, step=0)]
            ws = hip.workspace_for(cfg, n, th.device, nh)
            w = [1e4, 1e4, 1e4, 1e3]
            terms = hip.loss_forward(cfg, 0, th, x, nrm, sdf.reshape(-1), n, w, 100.0, ws, n_hess=nh)
            g = hip.loss_backward(cfg, 0, th, x, nrm, sdf.reshape(-1), n, w, 100.0, torch.ones(4, device="cuda"), None, ws, n_hess=nh)
            out["t%d" % n] = terms.cpu().numpy(); out["g%d" % n] = g.cpu().numpy()
        return out
    outs = {}
    for tag, opts in (("pair", {}), ("separate", {"pair_launch": 0}), ("quads_bf16", {"split_quads": 0})):
        with hip.options(**opts):
            outs[tag] = run()
    for n in (40000, 900):
        # the quads on bf16x6 (six products) instead of fp16x3: same tolerances, agreement far inside the Hessian term's noise
        assert rel(outs["pair"]["t%d" % n], outs["quads_bf16"]["t%d" % n]) < 5e-6, n
        assert rel(outs["pair"]["g%d" % n], outs["quads_bf16"]["g%d" % n]) < 2e-4, n
        assert rel(outs["pair"]["t%d" % n], outs["separate"]["t%d" % n]) < 2e-6, n
        # float atomics reorder the sums of d(theta); the Hessian term's own fp32 noise is 6e-5 (the reference's too)
        assert rel(outs["pair"]["g%d" % n], outs["separate"]["g%d" % n]) < 2e-5, n
    # the small case against the oracle (the large one costs minutes on the CPU)
    n = 900
    P = synth.siren_params([256] * 4, seed=31, dtype=np.float64)
    x, nrm, sdf = synth.training_batch(n, seed=6, step=0)
    terms, grads, _ = O.loss_and_grad("s1", P, x.astype(np.float64), nrm.astype(np.float64), sdf.astype(np.float64),
                                      [1e4, 1e4, 1e4, 1e3], 100.0)
    gref = np.concatenate([np.concatenate([w.reshape(-1), b.reshape(-1)]) for w, b in grads])
    for tag in ("pair", "separate", "quads_bf16"):
        assert rel(outs[tag]["t900"], np.array(list(terms.values()))) < 1e-5, tag
        assert rel(outs[tag]["g900"], gref) < 5e-4, tag
