# coding: utf-8
"""GPU: the map from a field value to a step length, `inverse(gt_mode, f, alpha, min_step)` (reference src/inverses.py:3-21), and
the hit / retire / accept rule behind it, in each of the four kernels that restate it — `field_features_kernel` (`grid_fields`,
`extract_fields`), `rays_step_kernel` (`trace_rays`), `rays_descend_kernel` (`descend_rays`) and `pc_step_kernel`
(`project_points`, `pointcloud_round`) — for 'tanh', 'siren' and 'squared'.

Networks: (T) the trained 4x128 `t_theta` of tests/golden/g14_pointcloud.npz, a distance field; (R) synth.siren_params([64]*3),
which takes both signs; (C) R with the last layer's weights zero and its bias c: the field is c everywhere, so every decision is
known exactly.  Bounds: u = 2^-24 is the unit roundoff of float32, 2^-52 twice that of float64; a float32 step is held to 4 u
relative of the exact float64 `inverse` of the SAME float32 field value (read back with `hip_ops.query`), 'siren' to its bits, the
float64 point-cloud step to 4 * 2^-52.  `oracle.rays_oracle.inverse` is the fixture-pinned restatement (tests/test_inverse_cpu.py)."""
import functools
import os

import numpy as np
import pytest
import torch

from diffudf_amd import synth
from oracle import rays_oracle as R, pointcloud_oracle as P

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MODES = ("tanh", "siren", "squared")
U32, E32, E64 = 2.0 ** -24, 4 * 2.0 ** -24, 4 * 2.0 ** -52
HID = {"T": [128] * 4, "R": [64] * 3}
ALPHA = {"T": 100.0, "R": 3.0}                       # R runs the alpha whose root is not a float32
THRESH = {"T": 0.05, "R": 0.2}
MIN_STEP = 0.003
# (alpha, surface threshold) of the constant-field cases.  347 is the smallest integer alpha at which the two 'tanh' branches differ
# in float32 AT the boundary b = float32(1/alpha) (sqrt(b / alpha) is one ulp from b; for 100 and 3, as for most alpha, they are
# the same float), so only there does the side the `<` takes show in the step.
EDGE_CASES = ((100.0, 0.004), (3.0, 0.05), (347.0, 0.001))
GRID_CAP_ROWS = 2048 * 256 + 300                     # rays_step_kernel strides past its launch cap of 2048 workgroups


@functools.lru_cache(maxsize=None)
def _params(net):
    if net == "T":
        G = np.load(os.path.join(HERE, "golden", "g14_pointcloud.npz"))
        return synth.unflatten_params(G["t_theta"].astype(np.float32), HID["T"])
    return synth.siren_params(HID["R"], seed=7)


def _const_params(c):
    p = list(_params("R"))
    p[-1] = (np.zeros_like(p[-1][0]), np.full_like(p[-1][1], np.float32(c)))
    return p


def _f64(params):
    return [(w.astype(np.float64), b.astype(np.float64)) for w, b in params]


def _dev(hidden, params):
    from diffudf_amd import hip_ops
    return hip_ops.make_cfg(hidden), torch.from_numpy(synth.flatten_params(params)).cuda()


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _query_twice(cfg, theta, x32, want_grad):
    """(f, g) as numpy from `hip_ops.query`; a second identical call must return the same bits."""
    from diffudf_amd import hip_ops
    f1, g1 = hip_ops.query(cfg, theta, _d(x32), want_grad=want_grad)
    f2, g2 = hip_ops.query(cfg, theta, _d(x32), want_grad=want_grad)
    assert torch.equal(f1, f2) and (not want_grad or torch.equal(g1, g2))
    return f1.cpu().numpy(), (g1.cpu().numpy() if want_grad else None)


def _same_nan(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b))


# ---- a. decision edges on constant fields ------------------------------------------------------------------------------------
def _lattice(m):
    """m rays: starts on a 4^3 lattice inside the box, seven fixed unit directions; a fifth of the rows enter with mask 0."""
    ax = np.array([-0.925, -0.3, 0.3, 0.925])
    pts = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    dirs = np.array([[1, 0, 0], [0, -1, 0], [0, 0, 1], [0.6, 0.8, 0], [0, -0.6, 0.8], [-0.8, 0, -0.6], [-0.36, 0.48, -0.8]], dtype=np.float64)
    i = np.arange(m)
    return dirs[i % 7].copy(), pts[i % 64].copy(), (i % 5 != 2)


def _edge_constants(mode, alpha, thr):
    """0, -0.2, +0.2, float32(1/alpha) with both neighbours, and one value whose step is just under / just over the threshold:
    'siren' compares the value itself (one float32 apart decides); the other two compare the float32 step, so the pair sits
    2^-19 relative (32 u) on either side — near, yet outside what a 4 u step error could flip."""
    f32 = np.float32
    b = f32(1 / alpha)
    if mode == "siren":
        under, over = np.nextafter(f32(thr), f32(0)), f32(thr)
    else:
        c0 = thr * thr * alpha                                  # sqrt(c0 / alpha) = thr on both branches used here
        assert c0 < 1 / alpha
        under, over = f32(c0 * (1 - 2.0 ** -18)), f32(c0 * (1 + 2.0 ** -18))
        for c, sign in ((under, -1), (over, 1)):
            s = float(R.inverse(mode, np.array([c], np.float64), alpha)[0])
            assert 8 * U32 < sign * (s / thr - 1) < 2.0 ** -17, (c, s, thr)
    return [f32(0), f32(-0.2), f32(0.2), np.nextafter(b, f32(0)), b, np.nextafter(b, f32(np.inf)), under, over]


def _expected_iterations(it_oracle, check_every, max_iterations):
    """The device looks at the active count every `check_every` iterations (and at the last one); the reference after each."""
    return min(max_iterations, max(check_every, -(-it_oracle // check_every) * check_every))


@pytest.mark.parametrize("mode", MODES)
def test_constant_field_decision_edges(mode):
    """Field = c everywhere (c_dev, read back from the device, must be c), alpha 100, 3 and 347 (EDGE_CASES): hits, mask and the iteration count of `trace_rays`
    equal `rays_oracle.propagate_rays` exactly, for check_every 1 and 3 and min_step 0.01 and 0.003, rows that enter with mask 0
    neither move nor hit, positions within 4 * 2^-52 * max|t0| per executed iteration (one FMA against numpy's two roundings);
    c = -0.2 under 'siren' hits at once through the signed test; c = 0 marches by min_step ('siren') or min_step / sqrt(alpha)
    ('squared').  `grid_fields` (N = 9, one call and two ragged ones) gives float32 inverse(|c|) — the reference's bits — and
    the hard-coded min_step 0.01 at c = 0.  `project_points(num_steps=1)`: zero gradient, so the point is NaN and rejected.
    Measured (MI355X): c_dev == c for every constant (an all-zero weight tensor passes the fp16x3 range scaling); all 108 traces
    per mode equal the oracle in hits, mask and iteration count; worst position error 0.06 of the allowance."""
    from diffudf_amd import hip_ops
    m, max_it = 257, 12
    rays, start, mask0 = _lattice(m)
    worst_pos, traces = 0.0, 0
    for alpha, thr in EDGE_CASES:
        for c in _edge_constants(mode, alpha, thr):
            params = _const_params(c)
            cfg, theta = _dev(HID["R"], params)
            f, _ = _query_twice(cfg, theta, start.astype(np.float32), False)
            c_dev = f[0]
            assert (f == c_dev).all() and c_dev == c and np.signbit(c_dev) == np.signbit(c), (c, c_dev)
            p64 = _f64(_const_params(c_dev))
            # -- trace_rays
            thresholds = [thr]
            if c == 0:
                thresholds.append(-1.0 if mode == "siren" else 1e-4)     # never close: the ray marches by min_step
            for th in thresholds:
                for ce in (1, 3):
                    for ms in (0.01, 0.003):
                        t_o, m_o = start.copy(), mask0.copy()
                        h_o, it_o = R.propagate_rays(p64, rays, t_o, m_o, mode, alpha, th, max_it, min_step=ms)
                        assert np.abs(np.abs(t_o) - 1).min() > 1e-9              # no oracle ray ends on the box's faces
                        d_t0, d_mask = _d(start.copy()), _d(mask0.astype(np.uint8))
                        hits, iters = hip_ops.trace_rays(cfg, theta, _d(rays), d_t0, d_mask, mode, alpha, th, max_it,
                                                         check_every=ce, min_step=ms)
                        t_d, m_d, h_d = d_t0.cpu().numpy(), d_mask.cpu().numpy().astype(bool), hits.cpu().numpy().astype(bool)
                        where = (mode, alpha, float(c), th, ce, ms)
                        assert np.array_equal(h_d, h_o) and np.array_equal(m_d, m_o), where
                        assert iters == _expected_iterations(it_o, ce, max_it), (where, iters, it_o)
                        assert np.array_equal(t_d[~mask0], start[~mask0]) and not h_d[~mask0].any() and not m_d[~mask0].any()
                        err = np.abs(t_d - t_o).max()
                        worst_pos = max(worst_pos, err / (E64 * max(it_o, 1) * np.abs(t_o).max()))
                        assert err <= E64 * max(it_o, 1) * max(np.abs(t_o).max(), np.abs(start).max()), (where, err)
                        traces += 1
                        if mode == "siren" and c < 0 and th > 0:
                            # every ray still inside after its first step is a hit of iteration 1: the test is udf < thr, signed
                            step = np.float64(np.abs(c_dev))                       # the step is |f|; only the hit test is signed
                            inside1 = (np.abs(start + rays * step) < 1).all(1)
                            assert it_o == 1 and np.array_equal(h_d, mask0 & inside1) and m // 3 < inside1.sum() < m, where
                        if c == 0 and th != thr:
                            step = R.inverse(mode, np.zeros(1, np.float32), alpha, ms)[0]
                            expect_step = np.float32(ms) if mode == "siren" else \
                                (np.float32(0) if mode == "tanh" else np.float32(np.float64(np.float32(ms)) / np.sqrt(alpha)))
                            assert step == expect_step
                            if mode != "tanh":                                   # 'tanh': step 0 is a hit where it stands
                                assert not h_d.any() and it_o == max_it
                                # row 0: from the corner cell along +x, never near a face within max_it steps
                                assert mask0[0] and m_d[0] and rays[0, 0] == 1
                                assert abs(t_d[0, 0] - (start[0, 0] + max_it * np.float64(step))) <= E64 * max_it
            # -- grid_fields, N = 9: one call and two ragged calls
            N = 9
            want = R.inverse(mode, np.abs(np.array([c_dev], np.float32)), alpha, 0.01)[0]
            exact = R.inverse(mode, np.abs(np.array([c_dev], np.float64)), alpha, 0.01)[0]
            assert want.dtype == np.float32
            for ranges in (((0, N ** 3),), ((0, 300), (300, N ** 3 - 300))):
                df = torch.full((N ** 3,), -7.0, device="cuda"); vec = torch.full((N ** 3, 3), -7.0, device="cuda")
                flagged = 0
                for s0, cnt in ranges:
                    flagged += int(hip_ops.grid_fields(cfg, theta, N, s0, cnt, mode, alpha, df, vec))
                got = df.cpu().numpy()
                assert (got == got[0]).all() and abs(float(got[0]) - exact) <= E32 * exact, (mode, alpha, c, got[0], want)
                assert got[0] == want, (mode, alpha, float(c), got[0], want)      # all three modes: the reference's float32 bits
                if c == 0:
                    assert got[0] == {"tanh": np.float32(0), "siren": np.float32(0.01),
                                      "squared": np.float32(np.float64(np.float32(0.01)) / np.sqrt(alpha))}[mode]
                assert flagged == N ** 3 and bool((vec == 0).all())               # zero gradient: every point takes the fallback flag
            # -- project_points, one step: the unit gradient is 0/0
            pts = _d(start.copy())
            last, unit, pre, acc = hip_ops.project_points(cfg, theta, pts, mode, alpha, 1, thr)
            assert bool(torch.isnan(pts).all()) and bool(torch.isnan(unit).all()) and int(acc.sum()) == 0, (mode, alpha, c)
            assert np.array_equal(pre.cpu().numpy(), start.astype(np.float32))
            with np.errstate(invalid="ignore"):
                want_last = R.inverse(mode, np.full(m, c_dev, np.float64), alpha, 0)
            got_last = last.cpu().numpy()
            assert _same_nan(got_last, want_last)
            ok = ~np.isnan(want_last)
            assert (np.abs(got_last[ok] - want_last[ok]) <= E64 * np.abs(want_last[ok])).all()
    print(f"\n[a] {mode}: {traces} traces equal the oracle in hits, mask and iteration count; worst position error "
          f"{worst_pos:.3f} of the allowance 4*2^-52*max|t0| per iteration")


# ---- b. one step on real networks ---------------------------------------------------------------------------------------------
def _inputs(m):
    rng = np.random.default_rng(1000 + m)
    t0 = rng.uniform(-0.98, 0.98, (m, 3))
    rays = rng.standard_normal((m, 3)); rays /= np.linalg.norm(rays, axis=1, keepdims=True)
    mask0 = rng.random(m) < 0.8
    sub = rng.random(m) < 0.5
    if m == 1:
        mask0[:] = True; sub[:] = True
    return rays, t0, mask0, sub


def _steps(mode, f, alpha, min_step):
    """(the step whose error is bounded, as float64; the relative bound; the float32 step of the reference)"""
    s32 = R.inverse(mode, np.abs(f), alpha, min_step)
    assert s32.dtype == np.float32
    if mode == "siren":
        return s32.astype(np.float64), 0.0, s32                  # bit-exact: the float32 value or float32(min_step)
    return R.inverse(mode, np.abs(f).astype(np.float64), alpha, min_step), E32, s32


def _check_trace_step(mode, net, m):
    from diffudf_amd import hip_ops
    cfg, theta = _dev(HID[net], _params(net))
    alpha, thr = ALPHA[net], THRESH[net]
    rays, t0, mask0, _ = _inputs(m)
    f, _ = _query_twice(cfg, theta, t0.astype(np.float32), False)
    step, rel, s32 = _steps(mode, f, alpha, MIN_STEP)
    d_t0, d_mask = _d(t0.copy()), _d(mask0.astype(np.uint8))
    hits, iters = hip_ops.trace_rays(cfg, theta, _d(rays), d_t0, d_mask, mode, alpha, thr, 1, check_every=1, min_step=MIN_STEP)
    q, m_d, h_d = d_t0.cpu().numpy(), d_mask.cpu().numpy().astype(bool), hits.cpu().numpy().astype(bool)
    assert iters == 1
    exp = t0 + rays * step[:, None]
    tol = rel * np.abs(rays) * step[:, None] + E64 * np.maximum(np.abs(t0), np.abs(exp))
    k = np.abs(rays).argmax(1); rows = np.arange(m)
    step_dev = (q[rows, k] - t0[rows, k]) / rays[rows, k]
    with np.errstate(invalid="ignore", divide="ignore"):
        rel_err = np.nan_to_num((np.abs(step_dev - step) / step)[mask0])
    # decisions: hit / retire from the reference's float32 comparison; rows within 4 u of a threshold or of a face are left out
    thr32 = np.float32(thr)
    quantity = f if mode == "siren" else np.abs(s32)
    close = quantity < thr32
    inside = (np.abs(exp) < 1).all(1)
    border = (np.abs(quantity.astype(np.float64) - float(thr32)) <= E32 * float(thr32)) | (np.abs(np.abs(exp) - 1) <= tol).any(1)
    judged = mask0 & ~border
    print(f"\n[b] trace {mode}/{net}/m={m}: worst relative step error {rel_err.max() if rel_err.size else 0:.2e} "
          f"(bound {rel:.2e} + recovery), rows left out {int((mask0 & border).sum())} of {int(mask0.sum())}, "
          f"hits {int(h_d.sum())}, retired {int((mask0 & ~m_d).sum())}, neg f {int((f < 0).sum())}")
    assert np.array_equal(q[~mask0], t0[~mask0]) and not h_d[~mask0].any() and not m_d[~mask0].any()
    assert (np.abs(q - exp)[mask0] <= tol[mask0]).all(), float((np.abs(q - exp) / tol)[mask0].max())
    assert (mask0 & border).sum() <= 0.005 * mask0.sum()
    assert np.array_equal(h_d[judged], (close & inside)[judged]) and np.array_equal(m_d[judged], (~close & inside)[judged])


@pytest.mark.parametrize("m", [1, 255, 256, 257, 4099])
@pytest.mark.parametrize("net", ["T", "R"])
@pytest.mark.parametrize("mode", MODES)
def test_one_step_on_real_networks(mode, net, m):
    """`trace_rays(max_iterations=1)`, `descend_rays(gd_steps=1)` on a random half of the rows and `project_points(num_steps=1)`
    against numpy updates formed from the device's own f (and g), read with `hip_ops.query` at float32(t0) for the same n.
    trace: |q - (t0 + ray step)| <= 4 u |ray| step + 4 * 2^-52 max|t0| ('siren': the first term is zero); descent: the
    displacement adds 4.5 u for the float32 normalisation (norm 2.5 u, quotient u, product u); point cloud: float64 without
    contraction, 4 * 2^-52 throughout.  Hits, retirements and accept flags equal the numpy decision except on rows whose decision
    quantity lies within 4 u of its threshold (or whose position lies within its bound of a face): at most 0.5 % of the rows.
    Rows outside `mask` / `hits` keep their bits.
    The marching loop, the descent and the projection see the bits `hip_ops.query` returns (same sweep variant: under 'siren' the
    step recovered from the positions is the queried value to 1e-13), so no allowance for a different f is made.
    Measured (MI355X), worst over the 10 cases of a mode: trace, relative step error against the exact map 7.5e-8 ('tanh'),
    1.0e-7 ('squared'), 1.4e-13 ('siren': what recovering a step from float64 positions leaves); descent, | |displacement| / step - 1 |
    1.7e-7, 2.0e-7, 1.4e-7; projection, step error 0 (numpy's bits); rows left out: none in any case."""
    from diffudf_amd import hip_ops
    _check_trace_step(mode, net, m)
    cfg, theta = _dev(HID[net], _params(net))
    alpha, thr = ALPHA[net], THRESH[net]
    _, t0, _, sub = _inputs(m)
    x32 = t0.astype(np.float32)
    f, g = _query_twice(cfg, theta, x32, True)
    g64 = g.astype(np.float64)
    unit = g64 / np.sqrt((g64 * g64).sum(1))[:, None]
    # -- descend_rays
    step, rel, _ = _steps(mode, f, alpha, MIN_STEP)
    d_t0 = _d(t0.copy())
    hip_ops.descend_rays(cfg, theta, d_t0, _d(sub.astype(np.uint8)), mode, alpha, 1, min_step=MIN_STEP)
    q = d_t0.cpu().numpy()
    disp = unit * step[:, None]
    tol = (rel + 4.5 * U32) * np.abs(disp) + E64 * np.abs(t0)
    moved = np.sqrt(((q - t0) ** 2).sum(1))
    with np.errstate(invalid="ignore", divide="ignore"):
        rel_err = np.nan_to_num((np.abs(moved - step) / step)[sub])
    print(f"[b] descend {mode}/{net}/m={m}: worst | |displacement| / step - 1 | {rel_err.max() if rel_err.size else 0:.2e}")
    assert np.array_equal(q[~sub], t0[~sub])
    assert (np.abs(q - (t0 - disp))[sub] <= tol[sub]).all(), float((np.abs(q - (t0 - disp)) / tol)[sub].max())
    # -- project_points
    pts = _d(t0.copy())
    last, d_unit, pre, acc = hip_ops.project_points(cfg, theta, pts, mode, alpha, 1, thr)
    s = t0.copy()
    with np.errstate(invalid="ignore"):
        steps = P.project_step(s, f, g, mode, alpha)
        want_acc = P.accept(s, steps, thr)
        got, got_last, got_acc = pts.cpu().numpy(), last.cpu().numpy(), acc.cpu().numpy().astype(bool)
        assert np.array_equal(pre.cpu().numpy(), x32)
        assert _same_nan(got_last, steps) and _same_nan(got, s) and np.array_equal(np.isnan(steps), (f < 0) & (mode == "tanh"))
        ok = ~np.isnan(steps)
        pc_rel = np.abs(got_last[ok] - steps[ok]) / np.where(steps[ok] == 0, 1, steps[ok])
        pos_tol = E64 * (np.abs(t0) + np.abs(steps)[:, None])
        border = (np.abs(steps - thr) <= E64 * thr) | (np.abs(np.abs(s) - 1) <= pos_tol).any(1)
        print(f"[b] project {mode}/{net}/m={m}: worst relative step error {pc_rel.max() if pc_rel.size else 0:.2e}, NaN rows "
              f"{int((~ok).sum())}, accepted {int(got_acc.sum())}, rows left out {int(border[ok].sum())}")
        assert (pc_rel <= E64).all()
        assert (np.abs(d_unit.cpu().numpy() - unit) <= E64).all()
        assert (np.abs(got - s)[ok] <= pos_tol[ok]).all()
        assert not got_acc[~ok].any() and border[ok].sum() <= 0.005 * m
        assert np.array_equal(got_acc[ok & ~border], want_acc[ok & ~border])


@pytest.mark.parametrize("mode", MODES)
def test_one_step_past_the_launch_cap(mode):
    """2048 * 256 + 300 rays, one iteration on (T): the rows behind the launch cap of `rays_step_kernel` (its grid stride) obey
    the same bounds and decisions as the rest.
    Measured (MI355X): relative step error 8.7e-8 ('tanh'), 9.5e-8 ('squared'), 1.2e-11 ('siren'); rows left out 1 of 419 849
    ('tanh', 'squared'), 0 ('siren')."""
    _check_trace_step(mode, "T", GRID_CAP_ROWS)


@pytest.mark.parametrize("net", ["T", "R"])
@pytest.mark.parametrize("mode", MODES)
def test_grid_fields_against_grid_values(mode, net):
    """`grid_fields` over a ragged range of a 12^3 grid against `inverse` of `grid_values` over the same range: within 4 u of
    the exact map ('siren' bit-exact), the reference's min_step 0.01, and nothing written outside the range.
    Measured (MI355X): worst relative error 7.3e-8 ('tanh'), 1.05e-7 ('squared'), 0 ('siren'); the reference's float32 bits on
    every point in all three modes."""
    from diffudf_amd import hip_ops
    cfg, theta = _dev(HID[net], _params(net))
    alpha, N, s0, cnt = ALPHA[net], 12, 101, 1003
    val = torch.full((N ** 3,), -7.0, device="cuda")
    hip_ops.grid_values(cfg, theta, N, s0, cnt, val)
    df = torch.full((N ** 3,), -7.0, device="cuda"); vec = torch.full((N ** 3, 3), -7.0, device="cuda")
    hip_ops.grid_fields(cfg, theta, N, s0, cnt, mode, alpha, df, vec)
    f, got, v = val.cpu().numpy(), df.cpu().numpy(), vec.cpu().numpy()
    out = np.ones(N ** 3, bool); out[s0:s0 + cnt] = False
    assert (f[out] == -7).all() and (got[out] == -7).all() and (v[out] == -7).all()
    f, got = f[~out], got[~out]
    step, rel, s32 = _steps(mode, f, alpha, 0.01)
    err = np.abs(got - step) / step
    print(f"\n[b] grid_fields {mode}/{net}: worst relative error {err.max():.2e} (bound {rel:.2e}), equal to the reference's float32 "
          f"bits on {np.mean(got == s32):.4f} of the points, neg f {int((f < 0).sum())}")
    assert (err <= rel).all()
    assert np.allclose(np.sqrt((v[~out].astype(np.float64) ** 2).sum(1)), 1.0, atol=1e-5)


# ---- c. whole loops against the fp64 oracle -----------------------------------------------------------------------------------
def _ray_set(n, seed=3):
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    d = -u + 0.25 * rng.standard_normal((n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d, 0.9 * u


@functools.lru_cache(maxsize=None)
def _oracle_rays(mode):
    rays, start = _ray_set(600)
    t0, mask = start.copy(), np.ones(len(start), bool)
    hits, it = R.propagate_rays(_f64(_params("T")), rays, t0, mask, mode, 100.0, 0.004, 150)
    t1 = t0.copy()
    R.grad_descent(_f64(_params("T")), t1, hits, mode, 100.0, 3)
    return hits, mask, t0, t1, it


@pytest.mark.parametrize("mode", MODES)
def test_whole_ray_loop_against_the_oracle(mode):
    """600 rays aimed at the shape from the sphere of radius 0.9, network (T), alpha 100, threshold 0.004: `trace_rays` to
    retirement (at most 150 iterations), then 3 `descend_rays` steps from the oracle's hit set and positions, against
    `rays_oracle.propagate_rays` / `grad_descent` in float64.  Allowances of tests/test_api_gpu.py for 'tanh': >= 99 % of the rays
    share their fate, those within 2e-3 after tracing, 1e-4 after descent.
    The oracle alone, float32 against float64 parameters (CPU): every fate equal in all three modes; positions after tracing
    within 1.9e-4 ('tanh'), 2.4e-4 ('siren'), 2.2e-6 ('squared'); after descent 5.8e-6, 1.4e-6, 4.4e-6.
    Measured (MI355X): every fate equal in all three modes (hits 340 / 396 / 364 of 600); positions after tracing within 2.1e-4
    ('tanh'), 8.4e-5 ('siren'), 3.9e-6 ('squared'); after descent 3.3e-6, 6.9e-7, 2.0e-6."""
    from diffudf_amd import hip_ops
    cfg, theta = _dev(HID["T"], _params("T"))
    rays, start = _ray_set(600)
    h_o, m_o, t_o, t1_o, it_o = _oracle_rays(mode)
    d_t0, d_mask = _d(start.copy()), torch.ones(len(start), dtype=torch.uint8, device="cuda")
    hits, iters = hip_ops.trace_rays(cfg, theta, _d(rays), d_t0, d_mask, mode, 100.0, 0.004, 150, check_every=4)
    h_d, m_d, t_d = hits.cpu().numpy().astype(bool), d_mask.cpu().numpy().astype(bool), d_t0.cpu().numpy()
    same = (h_d == h_o) & (m_d == m_o)
    dist = np.abs(t_d - t_o).max(1)
    d_t1 = _d(t_o.copy())
    hip_ops.descend_rays(cfg, theta, d_t1, _d(h_o.astype(np.uint8)), mode, 100.0, 3)
    t1_d = d_t1.cpu().numpy()
    print(f"\n[c] rays {mode}: iterations {iters} (oracle {it_o}), hits {int(h_d.sum())} (oracle {int(h_o.sum())}), still active "
          f"{int(m_d.sum())} ({int(m_o.sum())}), same fate {same.mean():.4f}, positions after tracing {dist[same].max():.2e}, "
          f"after descent {np.abs(t1_d - t1_o).max():.2e}")
    assert h_o.sum() > 200
    assert same.mean() >= 0.99
    assert dist[same].max() < 2e-3
    assert np.abs(t1_d - t1_o).max() < 1e-4
    assert np.array_equal(t1_d[~h_o], t_o[~h_o])


@pytest.mark.parametrize("mode", MODES)
def test_whole_projection_loop_against_the_oracle(mode):
    """`project_points`, 5 steps, on the 1500 start points of tests/golden/g14_pointcloud.npz, network (T), against
    `pointcloud_oracle.project_points` in float64.  Allowances of tests/test_pointcloud_gpu.py: >= 99 % share the accept flag,
    moved positions within 1e-4; NaN rows ('tanh', a negative value on the way) agree and are rejected.
    The oracle alone, float32 against float64 parameters (CPU): every accept flag and NaN row equal; moved positions within
    6.4e-5 ('tanh', 'siren'), 2.2e-6 ('squared').
    Measured (MI355X): every accept flag and NaN row equal (accepted 545 / 1308 / 105, 761 NaN rows under 'tanh'); moved positions
    within 6.9e-5 ('tanh', 'siren'), 3.5e-6 ('squared')."""
    from diffudf_amd import hip_ops
    G = np.load(os.path.join(HERE, "golden", "g14_pointcloud.npz"))
    cfg, theta = _dev(HID["T"], _params("T"))
    start = G["t_start"].copy()
    s = start.copy()
    steps, a_o, _ = P.project_points(_f64(_params("T")), s, mode, 100.0, 5, 0.01)
    pts = _d(start.copy())
    last, unit, pre, acc = hip_ops.project_points(cfg, theta, pts, mode, 100.0, 5, 0.01)
    got, a_d = pts.cpu().numpy(), acc.cpu().numpy().astype(bool)
    same = a_d == a_o
    nan_o, nan_d = np.isnan(s).any(1), np.isnan(got).any(1)
    ok = same & ~nan_o & ~nan_d
    err = np.abs(got - s)[ok].max()
    print(f"\n[c] points {mode}: accepted {int(a_d.sum())} (oracle {int(a_o.sum())}), NaN rows {int(nan_d.sum())} ({int(nan_o.sum())}), "
          f"same accept flag {same.mean():.4f}, moved positions {err:.2e}")
    assert same.mean() >= 0.99
    assert (nan_d == nan_o).mean() >= 0.99 and not a_d[nan_d].any()
    assert (nan_o.sum() > 0) == (mode == "tanh") and a_o.sum() > 50
    assert err < 1e-4


# ---- d. the Python surface in 'squared' ---------------------------------------------------------------------------------------
def _model():
    from diffudf_amd.model import SIREN
    m = SIREN(3, 1, HID["T"], w0=30).cuda()
    with torch.no_grad():
        m.flat_parameters().copy_(torch.from_numpy(synth.flatten_params(_params("T"))).cuda())
    return m


def test_python_surface_in_squared():
    """gt_mode 'squared' through the reference-named entry points: `src.render_st.propagate_rays` / `grad_descent` on 300 rays
    equal `hip_ops.trace_rays` / `descend_rays` bit for bit; `extract_fields(N=10)` equals one `grid_fields` call; and
    `Sampler.generate_point_cloud("squared", 100.0, num_points=777, rng="device")` returns >= 777 in-box rows with finite unit
    normals, twice the same arrays.
    Measured (MI355X): 183 of 300 rays hit; the cloud has 959 rows."""
    from diffudf_amd import hip_ops
    from src.render_st import propagate_rays, grad_descent
    from src.render_mc import extract_fields
    from src.render_pc import Sampler
    model = _model()
    cfg, theta = model.hip_cfg, model.flat_parameters()
    net_cfg = {"gt_mode": "squared", "alpha": 100.0}
    rcfg = {"surface_threshold": 0.004, "max_iterations": 100, "gd_steps": 3}
    rays, start = _ray_set(300, seed=5)
    t0, mask = start.copy(), np.ones(300, bool)
    hits = propagate_rays(model, rays, t0, mask, net_cfg, rcfg, "cuda:0")
    d_t0, d_mask = _d(start.copy()), torch.ones(300, dtype=torch.uint8, device="cuda")
    h_d, _ = hip_ops.trace_rays(cfg, theta, _d(rays), d_t0, d_mask, "squared", 100.0, 0.004, 100)
    assert hits.dtype == bool and hits.sum() > 100
    assert np.array_equal(hits, h_d.cpu().numpy().astype(bool)) and np.array_equal(mask, d_mask.cpu().numpy().astype(bool))
    assert np.array_equal(t0, d_t0.cpu().numpy())
    t1 = t0.copy()
    grad_descent(model, t1, hits, net_cfg, rcfg, "cuda:0")
    hip_ops.descend_rays(cfg, theta, d_t0, h_d, "squared", 100.0, 3)
    assert np.array_equal(t1, d_t0.cpu().numpy()) and not np.array_equal(t1[hits], t0[hits])
    # extract_fields
    N = 10
    df, vec = extract_fields(model, None, N, "squared", "cuda:0", 100.0)
    df2 = torch.empty(N ** 3, device="cuda"); vec2 = torch.empty(N ** 3, 3, device="cuda")
    flagged = int(hip_ops.grid_fields(cfg, theta, N, 0, N ** 3, "squared", 100.0, df2, vec2))
    assert df.shape == (N, N, N) and vec.shape == (N, N, N, 3) and df.dtype == torch.float32
    assert torch.equal(df.reshape(-1), df2) and flagged == 0 and torch.equal(vec.reshape(-1, 3), vec2)
    # the sampler
    s = Sampler.from_model(model)
    p0, n0 = s.generate_point_cloud("squared", 100.0, num_points=777, rng="device", seed=4)
    p1, n1 = s.generate_point_cloud("squared", 100.0, num_points=777, rng="device", seed=4)
    print(f"\n[d] squared: {int(hits.sum())} of 300 rays hit; point cloud of {len(p0)} rows")
    assert len(p0) >= 777 and p0.shape == n0.shape == (len(p0), 3) and p0.dtype == np.float64
    assert (np.abs(p0) <= 1).all() and np.isfinite(n0).all() and np.allclose(np.linalg.norm(n0, axis=1), 1.0, atol=1e-5)
    assert np.array_equal(p0, p1) and np.array_equal(n0, n1)
