# coding: utf-8
"""GPU: d(theta) PER PARAMETER TENSOR (and per band of 16 rows / columns of the hidden matrices) against the fp64 oracle, at the
sizes where the kernels change path — what one max-norm over the flat vector cannot see: the first layer's dW / db are 1e-2 ... 5e-2
of the largest entry of d(theta), so the 1e-4 bar on the flat vector lets 0.2 ... 1.4 % of error in them through.

  B  every loss (loss_s1 Eikonal / with the Hessian term, loss_s2, loss_siren) and fields_forward / fields_backward with seeded
     standard-normal cotangents, widths 32 ... 512 and a padded one (200 at 256), per tensor and per band;
  C  edge column counts of [256, 256] and [512, 512] — 1, 15 | 16 | 17, 127 | 128 | 129, 2047 | 2048 | 2049 points, and Hessian-path
     counts whose four columns per point end one before, on and one behind a 128-column pass — terms, d(theta) per tensor and
     (n <= 129) every stashed s, c, q, A, e, zbar of every column and layer, under the session's stash and (around 128) stash = 0;
  D  launch shapes of the weight-gradient path no other GPU test compares with the oracle: the three-buffer 24-bit GEMM, small /
     clamped column splits, the deterministic mode, the per-wave and transposed-read GEMMs, two uneven shards accumulated.
     Every case asserts that its branch is the one taken (stash mask, kernel choice, the launcher's column split restated in
     tests/parity_util.py).

Tolerances are the project's (tests/test_hip_parity.py): d(theta) 1e-4, 5e-4 with the Hessian term, terms 1e-5 (loss_s2: 2e-5), stash
5e-5 (s, c, q) and 2e-4 (A, e, zbar) — applied per tensor.  What they are set against, measured on the CPU: the oracle run in fp32
against itself in fp64 on the same inputs (worst tensor | worst band of a hidden matrix):
    B   Eikonal 2.8e-6 | 2.2e-6 ([200]*3), Hessian term 2.8e-5 | 3.5e-5 ([256]*3 n = 300), loss_s2 2.2e-6 | 1.8e-6, loss_siren
        7.9e-6 | 1.1e-5 ([200]*3), fields 1.8e-6 | 1.8e-6;  [64]*4 seed 11: 1.5e-5 (Hessian term), <= 3.6e-6 otherwise;
        [200]*3 seed 6: 2.7e-5 (Hessian term), <= 7.9e-6 otherwise
    C   [256, 256] seed 21: n_hess = 0 <= 1.3e-6, loss_s2 <= 1.3e-6, (n, n_hess) pairs <= 5.2e-6; stash <= 7.1e-6
        [512, 512] seed 22: n_hess = 0 <= 1.6e-6, loss_s2 <= 1.1e-6, (n, n_hess) pairs <= 1.3e-5; stash <= 1.5e-5
    D   [256]*3 n = 700 seed 13: Eikonal 1.8e-6, Hessian term 6.7e-6 (seed 8 gave 7.2e-5: not taken); n = 4000: 1.9e-6;
        [256]*8 n = 1000: 4.4e-6
so every case's fp32-oracle figure is below a quarter of its bar.  The band bar has no precedent: four times the fp32 oracle's worst
band over the cases of B, 4 x 3.53e-5 = 1.41e-4 (the margin covers the other summation order of atomics and split-K); no band may
be skipped (a band is skipped only when its reference is identically zero, which the caller-shaped gradient never is)."""
import numpy as np
import pytest
import torch

import parity_util as U

pytestmark = pytest.mark.gpu

BAND_TOL = U.BAND_TOL
TOL_F, TOL_G = 5e-6, 2e-5
TOL_STASH = {"s": 5e-5, "c": 5e-5, "q": 5e-5, "A": 2e-4, "e": 2e-4, "zbar": 2e-4}


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible")
    from diffudf_amd import hip_ops
    return hip_ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def tag(hidden, n, n_hess=None):
    return f"{hidden[0]}x{len(hidden)} n={n}" + ("" if n_hess is None else f" n_hess={n_hess}")


def step(hip, cfg, th, x, nrm, sdf, loss, n_hess=0, n_global=None, dtheta=None, stash_check=None):
    """terms and d(theta) of one loss on the device (numpy); stash_check(ws, after_backward) runs between and behind the two calls"""
    n = x.shape[0]
    ng = n if n_global is None else n_global
    mode = {"s1": hip.LOSS_S1, "s2": hip.LOSS_S2, "siren": hip.LOSS_SIREN}[U.LOSSES[loss][0]]
    w = U.LOSSES[loss][1]
    ws = hip.workspace_for(cfg, n, "cuda", n_hess=n_hess)
    xd, nd, sd = dev(x), dev(nrm), dev(sdf.reshape(-1))
    stats = None
    if loss == "s2":
        stats = hip.s2_forward_stats(cfg, th, xd, sd, ws)
        terms = hip.s2_terms(stats, w)
    else:
        terms = hip.loss_forward(cfg, mode, th, xd, nd, sd, ng, w, 100.0, ws, n_hess=n_hess)
    if stash_check:
        stash_check(ws, False)
    d = hip.loss_backward(cfg, mode, th, xd, nd, sd, ng, w, 100.0, torch.ones(4, device="cuda"), stats, ws, dtheta=dtheta,
                          accumulate=dtheta is not None, n_hess=n_hess)
    if stash_check:
        stash_check(ws, True)
    return terms.double().cpu().numpy(), d.double().cpu().numpy()


def check(case, loss, terms, d, ref, P, band=False):
    """terms, then every tensor of d(theta), then (band) every band of the hidden matrices against the oracle result `ref`; prints
    the case's line of the table"""
    t_ref, g_ref, _ = ref
    per = U.per_tensor_rel(d, g_ref, P)
    name, e = max(per, key=lambda t: t[1])
    bname, bd, skipped = U.worst_band(d, g_ref, P)
    et = U.rel(terms, t_ref) if terms is not None else 0.0
    print(f"dtheta-edges | {case} | {loss} | terms {et:.1e} | flat {U.rel(d, U.flat(g_ref)):.1e} | worst tensor {name} {e:.1e} | "
          f"worst band {bname} {bd}")
    assert np.isfinite(d).all(), f"{case} {loss}: d(theta) is not finite"
    if terms is not None:
        assert et < U.TOL_TERMS[loss], f"{case} {loss}: terms rel err {et:.2e} (bar {U.TOL_TERMS[loss]:.0e})"
    for nm, err in per:
        assert err < U.TOL_DTHETA[loss], f"{case} {loss}: {nm} rel err {err:.2e} (bar {U.TOL_DTHETA[loss]:.0e}); all: {per}"
    if band:
        assert skipped == 0, f"{case} {loss}: {skipped} bands with an all-zero reference"
        assert bd.err < BAND_TOL, f"{case} {loss}: {bname} band {bd} (bar {BAND_TOL:.2e})"


# ---- B: every loss, per tensor and per band, at small sizes -------------------------------------------------------------------------
def small_net(hip, hidden, seed):
    """(P64, cfg, theta on the device, unpad) — a width that is not built runs zero-padded at the next one; unpad maps the device's
    d(theta) to the caller's shapes"""
    P64, P32 = U.net(hidden, seed)
    cfg = hip.make_cfg(list(hidden))
    if cfg.hidden == hidden[0]:
        return P64, cfg, dev(U.flat(P32).astype(np.float32)), lambda d: d
    return P64, cfg, dev(U.pad_theta(P32, cfg.hidden)), lambda d: U.unpad_flat(d, P64, cfg.hidden)


@pytest.mark.parametrize("loss", list(U.LOSSES))
@pytest.mark.parametrize("hidden,n,seed", U.SMALL_NETS)
def test_every_loss_per_tensor_and_band(hip, hidden, n, seed, loss):
    P, cfg, th, unpad = small_net(hip, hidden, seed)
    x, nrm, sdf = U.thirds_batch(n, seed)
    n_hess = n // 3 if loss == "s1full" else 0
    assert (sdf[:n // 3, 0] == 0).all() and (sdf[n // 3:, 0] != 0).all()
    terms, d = step(hip, cfg, th, x, nrm, sdf, loss, n_hess=n_hess)
    check(tag(hidden, n), loss, terms, unpad(d), U.thirds_case(hidden, n, seed, loss), P, band=True)


@pytest.mark.parametrize("hidden,n,seed", U.SMALL_NETS)
def test_fields_backward_with_random_cotangents(hip, hidden, n, seed):
    P, cfg, th, unpad = small_net(hip, hidden, seed)
    x, _, _ = U.thirds_batch(n, seed)
    ybar, gbar = U.cotangents(n, seed)
    assert ybar.std() > 0.5 and gbar.std() > 0.5
    y_ref, g_ref, grads = U.fields_oracle(P, x, ybar, gbar)
    ws = hip.workspace_for(cfg, n, "cuda")
    xd = dev(x)
    f, g = hip.fields_forward(cfg, th, xd, ws)
    d = hip.fields_backward(cfg, th, xd, dev(ybar), dev(gbar), ws).double().cpu().numpy()
    ef, eg = U.rel(f.cpu().numpy(), y_ref), U.rel(g.cpu().numpy(), g_ref)
    assert ef < TOL_F and eg < TOL_G, f"{tag(hidden, n)} fields: f {ef:.2e} df/dx {eg:.2e}"
    check(tag(hidden, n), "fields", None, unpad(d), (None, grads, None), P, band=True)


# ---- C: edge column counts -----------------------------------------------------------------------------------------------------------
def stash_checker(hip, cfg, case, loss, n, n_hess, dbg):
    """compares what the sweeps stashed with the oracle's intermediates: s, c, q behind the forward call, A, e, zbar behind the
    backward call; Hessian-path points through the value channel of their quad (e there is the oracle's E, -E on the other points)"""
    L = cfg.n_hidden_layers

    def refs(after):
        for l in range(L):
            if not after:
                yield "s", l, dbg["cache"]["s"][l]
                yield "c", l, dbg["cache"]["c"][l]
                yield "q", l, dbg["rev"]["q"][l]
            else:
                tr = dbg["trace"]
                yield "A", l, tr["A"][l]
                if loss == "s1full":
                    e = np.array(tr["E"][l]); e[n_hess:] *= -1.0
                    yield "e", l, e
                else:
                    yield "e", l, tr["e"][l]
                yield "zbar", l, tr["zbar"][l]

    def run(ws, after):
        for name, l, ref in refs(after):
            got = hip.read_stash(cfg, name, l, n, ws).cpu().numpy()
            e = U.rel(got, ref)
            assert e < TOL_STASH[name], f"{case} {loss}: stash {name}[{l}] rel err {e:.2e} (bar {TOL_STASH[name]:.0e})"
    return run


def edge_run(hip, hidden, seed, n, n_hess):
    P, P32 = U.net(hidden, seed)
    cfg = hip.make_cfg(list(hidden))
    th = dev(U.flat(P32).astype(np.float32))
    x, nrm, sdf = U.edge_batch(n, n_hess, seed)
    assert (sdf[:n_hess, 0] == 0).all() and (n_hess == 0 or (sdf[n_hess:, 0] != 0).all())
    loss = "s1full" if n_hess else "s1eik"
    case = tag(hidden, n, n_hess) + f" stash {hip.stash_mode(cfg, n, n_hess)}"
    ref = U.edge_case(hidden, n, n_hess, seed, loss)
    sc = stash_checker(hip, cfg, case, loss, n, n_hess, ref[2]) if n <= 129 else None
    terms, d = step(hip, cfg, th, x, nrm, sdf, loss, n_hess=n_hess, stash_check=sc)
    check(case, loss, terms, d, ref, P)
    sdf2 = U.s2_sdf(sdf, n_hess)
    if sdf2 is not None:
        assert int((sdf2 == 0).sum()) >= 2
        terms, d = step(hip, cfg, th, x, nrm, sdf2, "s2")
        check(case, "s2", terms, d, U.edge_case(hidden, n, n_hess, seed, "s2"), P)


@pytest.mark.parametrize("n,n_hess", U.EDGE_SIZES)
@pytest.mark.parametrize("hidden,seed", U.EDGE_NETS)
def test_edge_column_counts(hip, hidden, seed, n, n_hess):
    edge_run(hip, hidden, seed, n, n_hess)


@pytest.mark.parametrize("n", [127, 128, 129])
@pytest.mark.parametrize("hidden,seed", U.EDGE_NETS)
def test_edge_column_counts_fp32_stash(hip, hidden, seed, n):
    with hip.options(stash=0):
        assert hip.stash_mode(hip.make_cfg(list(hidden)), n) == 0
        edge_run(hip, hidden, seed, n, 0)


# ---- D: launch shapes of the weight-gradient path -----------------------------------------------------------------------------------
def launch_net(hip, hidden=U.LAUNCH_NET, seed=U.LAUNCH_SEED):
    P, P32 = U.net(hidden, seed)
    return P, hip.make_cfg(list(hidden)), dev(U.flat(P32).astype(np.float32))


def launch_check(hip, case, n_hess, n=U.LAUNCH_N):
    P, cfg, th = launch_net(hip)
    loss = "s1full" if n_hess else "s1eik"
    terms, d = step(hip, cfg, th, *U.edge_batch(n, n_hess, U.LAUNCH_SEED), loss, n_hess=n_hess)
    check(f"{case} {tag(U.LAUNCH_NET, n, n_hess)}", loss, terms, d, U.edge_case(U.LAUNCH_NET, n, n_hess, U.LAUNCH_SEED, loss), P)


@pytest.mark.parametrize("n_hess", [0, 233])
def test_three_buffer_24bit_gemm(hip, n_hess):
    """option wgrad_buffers = 3: wgrad_hidden_f16p24_kernel<256,9>, which only a workspace with stash mask 7 gets"""
    _, cfg, _ = launch_net(hip)
    with hip.options(stash=7, wgrad_buffers=3):
        assert hip.stash_mode(cfg, U.LAUNCH_N, n_hess) == 7
        assert U.wgrad_kernel(cfg, U.LAUNCH_N, n_hess) == "wgrad_hidden_f16p24_kernel<256,9>"
        launch_check(hip, "wgrad_buffers=3", n_hess)
    assert U.wgrad_kernel(cfg, U.LAUNCH_N, n_hess) != "wgrad_hidden_f16p24_kernel<256,9>"       # (the default is another build)


@pytest.mark.parametrize("n_hess", [0, 233])
def test_small_workgroup_cap_splits_columns_in_four(hip, n_hess):
    with hip.options(wgrad_max_workgroups=8):
        assert hip.get_option("wgrad_max_workgroups") == 8 and hip.get_option("deterministic") == 0
        nsplit, steps, nj = U.wgrad_nsplit(256, 3, U.LAUNCH_N, n_hess, cap=8)
        assert (nsplit, nj) == (4, 2) and steps == (24 if n_hess == 0 else 48)
        launch_check(hip, "wgrad_max_workgroups=8", n_hess)


def test_small_workgroup_cap_with_more_layers_than_workgroups_allow_to_split(hip):
    """[256]*8: seven hidden matrices under a cap of 8 workgroups leave one column split"""
    hidden, n, seed = (256,) * 8, 1000, 123
    P, cfg, th = launch_net(hip, hidden, seed)
    with hip.options(wgrad_max_workgroups=8):
        assert hip.get_option("wgrad_max_workgroups") == 8
        nsplit, steps, nj = U.wgrad_nsplit(256, 8, n, 0, cap=8)
        assert (nsplit, nj, steps) == (1, 7, 32) and 8 // nj == 1
        terms, d = step(hip, cfg, th, *U.thirds_batch(n, seed), "s1eik")
    check(f"wgrad_max_workgroups=8 {tag(hidden, n)}", "s1eik", terms, d, U.thirds_case(hidden, n, seed, "s1eik"), P)


@pytest.mark.parametrize("n,n_hess,expect", [(700, 0, (24, 24)), (700, 233, (48, 48)), (4000, 0, (120, 128))])
def test_multi_gpu_workgroup_cap(hip, n, n_hess, expect):
    """240 workgroups (what a multi-GPU step sets): at 700 points the split is clamped to the 32-column steps there are, at 4000
    points 120 splits share 128 steps unevenly"""
    with hip.options(wgrad_max_workgroups=240):
        assert hip.get_option("wgrad_max_workgroups") == 240 and hip.get_option("deterministic") == 0
        assert U.wgrad_nsplit(256, 3, n, n_hess, cap=240)[:2] == expect
        launch_check(hip, "wgrad_max_workgroups=240", n_hess, n=n)


def test_column_split_clamped_to_the_steps_there_are(hip):
    """[256, 256] at 17 points under the default cap: 256 workgroups for one hidden matrix, but only 128 / 32 = 4 steps"""
    hidden, n, seed = (256, 256), 17, 3
    P, cfg, th = launch_net(hip, hidden, seed)
    cap = hip.get_option("wgrad_max_workgroups")
    nsplit, steps, nj = U.wgrad_nsplit(256, 2, n, 0, cap=cap)
    assert cap == 256 and nj == 1 and cap // nj > steps and nsplit == steps == 4 and hip.get_option("deterministic") == 0
    terms, d = step(hip, cfg, th, *U.thirds_batch(n, seed), "s1eik")
    check(f"nsplit clamped {tag(hidden, n)}", "s1eik", terms, d, U.thirds_case(hidden, n, seed, "s1eik"), P)


@pytest.mark.parametrize("n_hess", [0, 233])
def test_deterministic_mode_against_the_oracle(hip, n_hess):
    """one column split per weight tile, one block (one wave) over all columns in the thin-layer kernel"""
    with hip.options(deterministic=1):
        assert hip.get_option("deterministic") == 1
        assert U.wgrad_nsplit(256, 3, U.LAUNCH_N, n_hess, cap=hip.get_option("wgrad_max_workgroups"), deterministic=1)[0] == 1
        launch_check(hip, "deterministic=1", n_hess)


@pytest.mark.parametrize("n_hess", [0, 233])
@pytest.mark.parametrize("opt,kernel", [("wgrad_family", "wgrad_hidden_bf16_kernel<256>"), ("wgrad_tr", "wgrad_hidden_f16tr_kernel<256,9>")])
def test_per_wave_and_transposed_read_gemms(hip, opt, kernel, n_hess):
    """wgrad_family = 2 (bf16x6 per-wave split) and wgrad_tr = 1 (transposed fragment reads), both on fp32 rows: stash = 0"""
    _, cfg, _ = launch_net(hip)
    value = {"wgrad_family": 2, "wgrad_tr": 1}[opt]
    default = U.wgrad_kernel(cfg, U.LAUNCH_N, n_hess)
    with hip.options(stash=0, **{opt: value}):
        assert hip.get_option(opt) == value and hip.stash_mode(cfg, U.LAUNCH_N, n_hess) == 0
        assert U.wgrad_kernel(cfg, U.LAUNCH_N, n_hess) == kernel != default
        launch_check(hip, f"{opt}={value} stash=0", n_hess)


@pytest.mark.parametrize("n_hess,cut", [(233, 233), (0, 301)])
def test_two_uneven_shards_accumulated(hip, n_hess, cut):
    """shards [0, cut) and [cut, 700) of one batch (the first holds the Hessian-path points), each with n_global = 700, accumulated
    into ONE d(theta): the oracle's gradient of the whole batch"""
    n = U.LAUNCH_N
    P, cfg, th = launch_net(hip)
    x, nrm, sdf = U.edge_batch(n, n_hess, U.LAUNCH_SEED)
    loss = "s1full" if n_hess else "s1eik"
    ref = U.edge_case(U.LAUNCH_NET, n, n_hess, U.LAUNCH_SEED, loss)
    acc = torch.zeros_like(th)
    terms, first = np.zeros(4), None
    for a, b, nh in ((0, cut, n_hess), (cut, n, 0)):
        assert 0 < b - a != n and nh <= b - a
        t, d = step(hip, cfg, th, x[a:b], nrm[a:b], sdf[a:b], loss, n_hess=nh, n_global=n, dtheta=acc)
        terms += t
        first = d if first is None else first
    d = acc.double().cpu().numpy()
    # both shards arrived: the first one alone is far from the whole, and the second call added to it instead of overwriting
    assert U.rel(first, U.flat(ref[1])) > 0.05 and U.rel(d - first, U.flat(ref[1])) > 0.05
    check(f"shards 0:{cut}:{n} {tag(U.LAUNCH_NET, n, n_hess)}", loss, terms, d, ref, P)
