#!/usr/bin/env python
# coding: utf-8
"""Generate the golden fixtures in this directory by RUNNING THE REFERENCE ITSELF.

Run once, in the build container only (the reference is mounted read-only at
/root/reference and never travels to the GPU box):

    python tests/golden/make_golden.py

Inputs (weights, batches) come from `diffudf_amd.synth` (pure functions of a seed), so
the fixtures only have to carry seeds + the reference's OUTPUTS.  The reference modules
imported are exactly the hot path: src.model.SIREN, src.diff_operators.{gradient,hessian},
src.loss_functions.{loss_s1,loss_s2,loss_siren}, src.evaluate.evaluate, src.inverses.inverse,
plus torch.optim.Adam as the reference's train loop uses it (train.py:334-337, :195-222).
"""
import os
import sys
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, "/root/reference")          # `src.*` must resolve to the REFERENCE here, not to this repo's shim
sys.path.append(REPO)
sys.path[:] = [p for p in sys.path if os.path.abspath(p or ".") != REPO] + [REPO]

from src.model import SIREN                                     # noqa: E402  (reference)
from src.diff_operators import gradient, hessian, jacobian      # noqa: E402  (reference)
from src.loss_functions import loss_s1, loss_s2, loss_siren     # noqa: E402  (reference)
from src.evaluate import evaluate                               # noqa: E402  (reference)
from src.inverses import inverse                                # noqa: E402  (reference)
from diffudf_amd import synth                                   # noqa: E402

torch.set_num_threads(8)


def ref_model(hidden, params, dtype):
    m = SIREN(3, 1, hidden, w0=30)
    sd = {}
    for i, (w, b) in enumerate(params):
        sd[f"net.{i}.0.weight"] = torch.from_numpy(np.asarray(w, dtype=np.float64))
        sd[f"net.{i}.0.bias"] = torch.from_numpy(np.asarray(b, dtype=np.float64))
    m = m.double()
    m.load_state_dict(sd)
    return m.to(dtype)


def flat_grads(model):
    return np.concatenate([p.grad.detach().reshape(-1).double().numpy() for p in model.parameters()])


def run_losses(hidden, params, batch, dtype, tag, out, sample=None):
    x, nrm, sdf = [torch.from_numpy(a.astype(np.float64)).to(dtype)[None] for a in batch]
    model = ref_model(hidden, params, dtype)
    # value / gradient / hessian exactly as src/evaluate.py:26-32 obtains them
    mo = model(x)
    xin, y = mo["model_in"], mo["model_out"]
    g = gradient(y, xin)
    H = hessian(y, xin)
    out[f"{tag}_y"] = y.detach().double().numpy()[0, :, 0]
    out[f"{tag}_g"] = g.detach().double().numpy()[0]
    out[f"{tag}_H"] = H.detach().double().numpy()[0]
    gt = {"normals": nrm, "sdf": sdf}
    cases = {
        "s1eik": (loss_s1, [1e4, 1e4, 0.0, 1e3], True),
        "s1full": (loss_s1, [1e4, 1e4, 1e4, 1e3], True),
        "s2": (loss_s2, [1e5, 1e5], True),
        "siren": (loss_siren, [3e3, 1e2, 1e2, 5e1], False),
    }
    for name, (fn, w, has_alpha) in cases.items():
        model.zero_grad()
        terms = fn(model, x, gt, w, 100) if has_alpha else fn(model, x, gt, w)
        total = torch.zeros((1, 1), dtype=dtype)
        for v in terms.values():
            total = total + v
        total.backward()
        out[f"{tag}_{name}_terms"] = np.array([float(v) for v in terms.values()])
        gr = flat_grads(model)
        if sample is None:
            out[f"{tag}_{name}_dtheta"] = gr
        else:
            out[f"{tag}_{name}_dtheta_sample"] = gr[sample]
            out[f"{tag}_{name}_dtheta_norm"] = np.array([np.linalg.norm(gr), np.abs(gr).max()])


def trajectory(hidden, params, n_pts, steps, lr, mode, weights, dtype, seed):
    """N Adam steps the way train.py:195-222 runs them (zero_grad, loss dict, sum, backward, step)."""
    model = ref_model(hidden, params, dtype)
    opt = torch.optim.Adam(lr=lr, params=model.parameters())
    fn = {"s1": loss_s1, "s2": loss_s2}[mode]
    hist = []
    for t in range(steps):
        x, nrm, sdf = [torch.from_numpy(a.astype(np.float64)).to(dtype)[None]
                       for a in synth.training_batch(n_pts, seed=seed, step=t, dtype=np.float64)]
        opt.zero_grad()
        terms = fn(model, x, {"normals": nrm, "sdf": sdf}, weights, 100)
        total = torch.zeros((1, 1), dtype=dtype)
        for v in terms.values():
            total = total + v
        total.backward()
        opt.step()
        hist.append([float(v) for v in terms.values()])
    theta = np.concatenate([p.detach().reshape(-1).double().numpy() for p in model.parameters()])
    return np.array(hist), theta


def make_g6():
    """G6: normals + curvatures at query points the way the sphere tracer derives them (reference
    src/render_st.py:57-62 `compute_normals_and_cd`, :42-55 `compute_curvature`; that module itself needs open3d,
    so its few torch lines are issued here against the imported `hessian` / `jacobian` / torch.linalg.eigh)."""
    out = {}
    for tag, hid, pseed, n in (("tiny", [32, 32, 32], 11, 48), ("full", [256] * 8, 123, 40)):
        P = synth.siren_params(hid, seed=pseed, dtype=np.float64)
        x64 = synth.uniform01(77, 601, 0, 3 * n).reshape(n, 3) * 1.6 - 0.8
        out[f"{tag}_hidden"] = np.array(hid); out[f"{tag}_param_seed"] = pseed; out[f"{tag}_x"] = x64.astype(np.float32)
        for dt, dn in ((torch.float64, "f64"), (torch.float32, "f32")):
            model = ref_model(hid, P, dt)
            x = torch.from_numpy(x64.astype(np.float32).astype(np.float64)).to(dt)[None]
            mo = model(x)
            xin, y = mo["model_in"], mo["model_out"]
            Hs = hessian(y, xin)                                            # render_st.py:58
            lam, V = torch.linalg.eigh(Hs)                                  # :59
            nrm = V[..., 2]                                                 # :60
            shape_op, status = jacobian(nrm, xin)                           # :43
            assert status == 0
            mean = torch.sum(torch.diagonal(shape_op[0], dim1=1, dim2=2), dim=-1) / 2          # :45
            ext = torch.zeros((shape_op.shape[1], 4, 4), dtype=dt)          # :48-53
            ext[:, :3, :3] = shape_op[0]
            ext[:, :3, 3] = nrm[0]
            ext[:, 3, :3] = nrm[0]
            gauss = -1 * torch.linalg.det(ext)
            for k, v in (("H", Hs[0]), ("lam", lam[0]), ("n", nrm[0]), ("pcd", V[0][..., :2]), ("shape_op", shape_op[0]),
                         ("mean", mean), ("gauss", gauss)):
                out[f"{tag}_{dn}_{k}"] = v.detach().double().numpy()
    np.savez_compressed(os.path.join(HERE, "g6_curvature.npz"), **out)


def make_g7():
    """G7: the sphere-tracing loop (reference src/render_st.py:136-172 `propagate_rays`, `grad_descent`; the module needs
    open3d, so its numpy bookkeeping is re-issued here around the REFERENCE model, gradient() and inverse()): rays start
    on the plane z = 0.95 and head into the domain."""
    from src.util import normalize                                   # reference
    out = {}
    for tag, hid, pseed in (("tiny", [32, 32, 32], 11), ("full", [256] * 8, 123)):
        P = synth.siren_params(hid, seed=pseed, dtype=np.float64)
        model = ref_model(hid, P, torch.float32)
        side = 24
        gx, gy = np.meshgrid(np.linspace(-0.8, 0.8, side), np.linspace(-0.8, 0.8, side), indexing="ij")
        t0 = np.stack([gx.ravel(), gy.ravel(), np.full(side * side, 0.95)], 1)
        rays = np.stack([0.15 * gx.ravel(), -0.1 * gy.ravel(), -np.ones(side * side)], 1)
        rays /= np.linalg.norm(rays, axis=1, keepdims=True)
        mask = np.ones(side * side, dtype=bool)
        cfg = {"gt_mode": "tanh", "alpha": 100, "surface_threshold": 0.004, "max_iterations": 40, "gd_steps": 3}
        out[f"{tag}_hidden"] = np.array(hid); out[f"{tag}_param_seed"] = pseed
        out[f"{tag}_rays"] = rays.copy(); out[f"{tag}_t0"] = t0.copy()
        for k in ("alpha", "surface_threshold", "max_iterations", "gd_steps"):
            out[f"{tag}_{k}"] = cfg[k]

        def query(pts, want_grad):
            mo = model(torch.from_numpy(pts).float()[None])
            y = mo["model_out"]
            g = gradient(y, mo["model_in"])[0].detach().numpy() if want_grad else None
            return y[0].detach().numpy(), g

        hits = np.zeros_like(mask)
        it = 0
        while mask.sum() > 0 and it < cfg["max_iterations"]:
            udfs, _ = query(t0[mask], False)
            steps = inverse(cfg["gt_mode"], np.abs(udfs), cfg["alpha"])
            t0[mask] += rays[mask] * steps
            close = np.abs(steps).flatten() < cfg["surface_threshold"]
            inside = np.logical_and(np.all(t0[mask] > -1, axis=1), np.all(t0[mask] < 1, axis=1))
            hits[mask] += np.logical_and(close, inside)
            mask[mask] *= np.logical_and(np.logical_not(close), inside)
            it += 1
        out[f"{tag}_hits"] = hits.copy(); out[f"{tag}_mask"] = mask.copy(); out[f"{tag}_t0_traced"] = t0.copy()
        out[f"{tag}_iterations"] = it
        for _ in range(cfg["gd_steps"]):
            udfs, g = query(t0[hits], True)
            steps = inverse(cfg["gt_mode"], np.abs(udfs), cfg["alpha"])
            t0[hits] -= normalize(g) * steps
        out[f"{tag}_t0_descended"] = t0.copy()
    np.savez_compressed(os.path.join(HERE, "g7_rays.npz"), **out)


def make_g8():
    """G8: small operator fixtures — reference src/util.py:34-39 `normalize` (1-D and per-row 2-D), reference
    src/diff_operators.py:196-205 `laplace` / `divergence` of the model's own gradient field."""
    from src.util import normalize                                   # reference
    from src.diff_operators import laplace, divergence               # reference
    out = {}
    v = synth.uniform01(5, 801, 0, 21).reshape(7, 3) * 4.0 - 2.0
    out["norm_in_2d"] = v; out["norm_out_2d"] = normalize(v)
    out["norm_in_1d"] = v[2].copy(); out["norm_out_1d"] = normalize(v[2].copy())
    for tag, hid, pseed, n in (("tiny", [32, 32, 32], 11, 48), ("full", [256] * 8, 123, 40)):
        P = synth.siren_params(hid, seed=pseed, dtype=np.float64)
        x64 = synth.uniform01(77, 601, 0, 3 * n).reshape(n, 3) * 1.6 - 0.8        # the points of G6
        model = ref_model(hid, P, torch.float64)
        x = torch.from_numpy(x64.astype(np.float32).astype(np.float64))[None]
        mo = model(x)
        lap = laplace(mo["model_out"], mo["model_in"])
        g = gradient(mo["model_out"], mo["model_in"])
        div = divergence(g, mo["model_in"])
        out[f"{tag}_laplace"] = lap.detach().numpy()[0]; out[f"{tag}_div_grad"] = div.detach().numpy()[0]
    np.savez_compressed(os.path.join(HERE, "g8_operators.npz"), **out)


def make_g9():
    """G9: the field slice of reference generate_df.py:50-107 (`generate_df`; the script needs open3d, so its numpy/torch
    lines are issued here around the REFERENCE `evaluate`, `normalize` and torch.linalg.eigh): sample plane, predicted
    value, |grad f|, and the normal map before colouring.  48 x 48 samples, SIREN 8x256 from the synth generator."""
    from src.util import normalize                                   # reference
    out = {}
    hid, W = [256] * 8, 48
    P = synth.siren_params(hid, seed=123, dtype=np.float64)
    model = ref_model(hid, P, torch.float32)
    BORDES, EJEPLANO, OFFSETPLANO = [1, -1], [2, 1, 0], 0.0
    ranges = np.linspace(BORDES[0], BORDES[1], W)
    i_1, i_2 = np.meshgrid(ranges, ranges)
    samples = np.concatenate(np.concatenate(np.array([np.expand_dims(i_1, 2), np.expand_dims(i_2, 2),
                                                      np.expand_dims(np.ones_like(i_1) * OFFSETPLANO, 2)])[EJEPLANO], axis=2), axis=0)
    gradients = np.zeros((W * W, 3)); hessians = np.zeros((W * W, 3, 3))
    pred = evaluate(model, samples, device=torch.device("cpu"), gradients=gradients, hessians=hessians)
    gnorm = np.linalg.norm(gradients, axis=1).reshape((-1, 1))
    g = normalize(gradients)
    lam, V = torch.linalg.eigh(torch.from_numpy(hessians))
    pn = V[..., 2].numpy()
    pn = np.where(np.sum(g * pn, axis=-1)[..., None] < 0, np.ones((len(pn), 1)) * -1, np.ones((len(pn), 1))) * pn
    normals = np.where(np.concatenate([gnorm, gnorm, gnorm], axis=-1) < 0.04, pn, g)
    normals = normals * np.hstack([np.ones((len(normals), 2)), np.sign(normals[:, 2]).reshape((len(normals), 1))])
    out["width"] = np.array(W); out["samples"] = samples; out["pred_distances"] = pred; out["pred_grad_norm"] = gnorm
    out["normals"] = normals; out["grad_map_u8"] = (((normals + 1) / 2).reshape(W, W, 3) * 255).astype(np.uint8)
    out["hidden"] = np.array(hid); out["param_seed"] = np.array(123)
    np.savez_compressed(os.path.join(HERE, "g9_slice.npz"), **out)


def meshudf_case(kind, n, seed):
    """Analytic unsigned fields + direction fields (what `extract_fields` hands to the MeshUDF extraction: |f| and the
    NEGATED normalised gradient), float32."""
    ax = np.linspace(-1, 1, n)
    A, B, C = np.meshgrid(ax, ax, ax, indexing="ij")
    rng = np.random.default_rng(seed)
    if kind == "sphere":
        r = np.sqrt(A * A + B * B + C * C); sd = r - 0.6
        g = np.stack([A, B, C], -1) / np.maximum(r, 1e-9)[..., None]
    elif kind == "sheet":                                   # open surface that leaves the domain
        ga = -0.45 * np.cos(3 * A) * np.cos(2 * B); gb = 0.30 * np.sin(3 * A) * np.sin(2 * B)
        nrm = np.sqrt(ga * ga + gb * gb + 1); sd = (C - 0.15 * np.sin(3 * A) * np.cos(2 * B)) / nrm
        g = np.stack([ga, gb, np.ones_like(ga)], -1) / nrm[..., None]
    elif kind == "cap":                                     # surface with a boundary inside the domain
        r = np.sqrt(A * A + B * B + C * C); sd = r - 0.7
        g = np.stack([A, B, C], -1) / np.maximum(r, 1e-9)[..., None]
        sd = np.where(C < -0.2, np.abs(sd) + (-0.2 - C), sd)
    elif kind == "two":                                     # two spheres meeting: ambiguous Lewiner configurations
        r1 = np.sqrt((A - 0.33) ** 2 + B * B + C * C); r2 = np.sqrt((A + 0.33) ** 2 + B * B + C * C)
        s1, s2 = r1 - 0.36, r2 - 0.36
        sd = np.minimum(s1, s2)
        g1 = np.stack([A - 0.33, B, C], -1) / np.maximum(r1, 1e-9)[..., None]
        g2 = np.stack([A + 0.33, B, C], -1) / np.maximum(r2, 1e-9)[..., None]
        g = np.where((s1 < s2)[..., None], g1, g2)
    elif kind == "noisy":                                   # unreliable gradients: the unsure / deferred queues
        r = np.sqrt(A * A + B * B + C * C); sd = r - 0.55 + 0.04 * np.sin(9 * A) * np.sin(8 * B) * np.sin(7 * C)
        g = np.stack([A, B, C], -1) / np.maximum(r, 1e-9)[..., None] + 0.25 * rng.standard_normal(A.shape + (3,))
        g = g / np.linalg.norm(g, axis=-1, keepdims=True)
    elif kind == "zeros":                                   # exact zeros in the field, zero gradients at 5 % of the points
        r = np.sqrt(A * A + B * B + C * C); sd = r - 0.5
        g = np.stack([A, B, C], -1) / np.maximum(r, 1e-9)[..., None]
        sd = np.where(np.abs(sd) < 0.03, 0.0, sd)
        g = np.where((rng.random(A.shape) < 0.05)[..., None], 0.0, g)
    udf = np.abs(sd).astype(np.float32)
    return udf, (-g * np.sign(sd)[..., None]).astype(np.float32)


def make_g10():
    """MeshUDF marching cubes: the reference's own Cython extension, rebuilt from its sources where
    they lie (oracle/build_ref.py -> oracle/_ref/), run through the reference's own wrapper `udf_mc_lewiner` on analytic
    fields.  Inputs: field, direction field, and the look-up tables AS THE WRAPPER PASSES THEM to the extension (the
    extension's `luts` argument, decoded by the reference's `_to_array`).  Outputs: vertices, faces, normals, values."""
    sys.path.insert(0, REPO)
    from oracle import build_ref
    ref = build_ref.load()
    assert ref is not None, "needs /root/reference and Cython"
    import _marching_cubes_lewiner_luts as mcluts
    out = {}
    names = [n for n in dir(mcluts) if n.isupper() and isinstance(getattr(mcluts, n), tuple)]
    for nme in names:
        out["lut_" + nme] = ref._to_array(getattr(mcluts, nme)).copy()
    for nme, arr in (("EDGESRELX", ref.EDGETORELATIVEPOSX), ("EDGESRELY", ref.EDGETORELATIVEPOSY), ("EDGESRELZ", ref.EDGETORELATIVEPOSZ)):
        out["lut_" + nme] = np.asarray(arr, np.int8)
    cases = [("sphere", 14, 0), ("sheet", 16, 0), ("cap", 18, 0), ("two", 20, 0), ("noisy", 17, 3), ("zeros", 19, 4), ("noisy", 24, 9)]
    out["cases"] = np.array([f"{k}_{n}_{s}" for k, n, s in cases])
    for k, n, s in cases:
        udf, g = meshudf_case(k, n, s)
        v, f, nn, val = ref.udf_mc_lewiner(udf, g, spacing=[2.0 / (n - 1)] * 3, avg_thresh=1.05, max_thresh=1.75)
        tag = f"{k}_{n}_{s}"
        out[tag + "_udf"] = udf; out[tag + "_grads"] = g
        out[tag + "_vertices"] = v; out[tag + "_faces"] = f.astype(np.int32); out[tag + "_normals"] = nn; out[tag + "_values"] = val
        print(tag, v.shape, f.shape)
    np.savez_compressed(os.path.join(HERE, "g10_meshudf.npz"), **out)


def make_g13():
    """MeshUDF marching cubes on the randomised fields of tests/test_meshudf.py: the reference's own extension (as in g10),
    recorded as digests of its outputs (the meshes themselves would be megabytes), of the fields it ran on and of its tables."""
    sys.path.insert(0, REPO)
    from oracle import build_ref
    ref = build_ref.load()
    assert ref is not None, "needs the reference sources and Cython"
    sys.path.insert(0, os.path.dirname(HERE))
    from test_meshudf import digest, random_fields
    from diffudf_amd import marching_cubes as mc
    luts = mc.load_luts()                                   # the reference's table module, decoded as its wrapper does
    inputs, outputs = [], []
    for trial, udf, gg, sp in random_fields():
        inputs.append(digest(udf, gg))
        try:
            v, f, nn, val = ref.udf_mc_lewiner(udf, gg, spacing=sp)
            outputs.append(digest(f, v, val, nn))
        except RuntimeError:
            outputs.append("RuntimeError")
        print(trial, udf.shape[0], outputs[-1][:16])
    np.savez_compressed(os.path.join(HERE, "g13_meshudf_random.npz"), input_digests=np.array(inputs), output_digests=np.array(outputs),
                        lut_digest=np.array(digest(*(luts[k] for k in mc.LUT_NAMES))))


def make_g11():
    """G11 (round 4): the two constructor arguments no shipped config uses but the reference's model accepts.
      ww: SIREN(3, 1, hidden, w0=30, ww=15) — first SineLayer at w0, the others at ww (reference src/model.py:89-106): value,
          df/dx, Hessian, the loss_s1 terms (Eikonal and full) and d(theta), fp64 and fp32 runs.  Hidden weights are drawn with
          the bound the reference's `sine_init(ww)` uses.
      latent: SIREN(3 + k, 1, hidden) queried through the reference's own `evaluate(model, samples, latent_vec, ...)`
          (src/evaluate.py:5-36): values and gradients[..., k:]."""
    out = {}
    for tag, hid, pseed, n in (("tiny", [32, 32, 32], 5, 96), ("full", [256] * 8, 123, 300)):
        P = synth.siren_params(hid, seed=pseed, w0=15.0, dtype=np.float64)       # sine_init(ww): hidden bound sqrt(6/fan)/ww
        batch = synth.training_batch(n, seed=pseed + 1, dtype=np.float64)
        out[f"ww_{tag}_hidden"] = np.array(hid); out[f"ww_{tag}_param_seed"] = pseed; out[f"ww_{tag}_n"] = n
        for dt, dn in ((torch.float64, "f64"), (torch.float32, "f32")):
            model = SIREN(3, 1, hid, w0=30, ww=15).double()
            model.load_state_dict({f"net.{i}.0.{k}": torch.from_numpy(np.asarray(a, dtype=np.float64))
                                   for i, (w, b) in enumerate(P) for k, a in (("weight", w), ("bias", b))})
            model = model.to(dt)
            x, nrm, sdf = [torch.from_numpy(a.astype(np.float32).astype(np.float64)).to(dt)[None] for a in batch]
            mo = model(x)
            xin, y = mo["model_in"], mo["model_out"]
            out[f"ww_{tag}_{dn}_y"] = y.detach().double().numpy()[0, :, 0]
            out[f"ww_{tag}_{dn}_g"] = gradient(y, xin).detach().double().numpy()[0]
            out[f"ww_{tag}_{dn}_H"] = hessian(y, xin).detach().double().numpy()[0]
            for name, w in (("s1eik", [1e4, 1e4, 0.0, 1e3]), ("s1full", [1e4, 1e4, 1e4, 1e3])):
                model.zero_grad()
                terms = loss_s1(model, x, {"normals": nrm, "sdf": sdf}, w, 100)
                total = torch.zeros((1, 1), dtype=dt)
                for v in terms.values():
                    total = total + v
                total.backward()
                out[f"ww_{tag}_{dn}_{name}_terms"] = np.array([float(v) for v in terms.values()])
                gr = flat_grads(model)
                if tag == "tiny":
                    out[f"ww_{tag}_{dn}_{name}_dtheta"] = gr
                else:                                        # 461 825 parameters: every 97th + the norms
                    out[f"ww_{tag}_{dn}_{name}_dtheta_sample"] = gr[::97]
                    out[f"ww_{tag}_{dn}_{name}_dtheta_norm"] = np.array([np.linalg.norm(gr), np.abs(gr).max()])
    # latent vector: k extra input features in FRONT of the coordinates (src/evaluate.py:21-22)
    k = 5
    for tag, hid, pseed, n in (("tiny", [32, 32, 32], 9, 80), ("full", [256] * 8, 321, 200)):
        P = synth.siren_params(hid, seed=pseed, n_in=3 + k, dtype=np.float64)
        lat = (synth.uniform01(pseed, 77, 0, k) * 2.0 - 1.0)[None, :]
        xs = (synth.uniform01(pseed, 78, 0, 3 * n).reshape(n, 3) * 2.0 - 1.0).astype(np.float32)
        out[f"lat_{tag}_hidden"] = np.array(hid); out[f"lat_{tag}_param_seed"] = pseed; out[f"lat_{tag}_k"] = k
        out[f"lat_{tag}_latent"] = lat; out[f"lat_{tag}_x"] = xs
        for dt, dn in ((torch.float64, "f64"), (torch.float32, "f32")):
            model = SIREN(3 + k, 1, hid, w0=30).double()
            model.load_state_dict({f"net.{i}.0.{kk}": torch.from_numpy(np.asarray(a, dtype=np.float64))
                                   for i, (w, b) in enumerate(P) for kk, a in (("weight", w), ("bias", b))})
            model = model.to(dt)
            # (no `hessians=`: the reference's hessian() differentiates the first three INPUT features — latent components here —
            #  and its evaluate() then fails with a shape error, src/diff_operators.py:187-193, src/evaluate.py:32)
            grads = np.zeros((n, 3))
            samples = torch.from_numpy(xs.astype(np.float64)).to(dt)
            vals = evaluate(model, samples, latent_vec=torch.from_numpy(lat).to(dt), max_batch=64, device=torch.device("cpu"),
                            gradients=grads)
            out[f"lat_{tag}_{dn}_y"] = vals[:, 0]; out[f"lat_{tag}_{dn}_g"] = grads
    np.savez_compressed(os.path.join(HERE, "g11_ww_latent.npz"), **out)
    print("g11_ww_latent.npz:", len(out), "arrays")


def main():
    # ---- G1: tiny net, everything stored --------------------------------------------------
    out = {}
    hid = [32, 32, 32]
    p64 = synth.siren_params(hid, seed=7, dtype=np.float64)
    batch = synth.training_batch(63, seed=7, dtype=np.float64)
    out["hidden"] = np.array(hid)
    out["param_seed"] = np.array(7); out["batch_seed"] = np.array(7); out["n_points"] = np.array(63)
    run_losses(hid, p64, batch, torch.float64, "f64", out)
    # the fp32 run uses fp32-rounded weights and inputs (what a user of the reference has)
    p32 = [(w.astype(np.float32), b.astype(np.float32)) for w, b in p64]
    b32 = [a.astype(np.float32) for a in batch]
    run_losses(hid, p32, b32, torch.float32, "f32", out)
    np.savez_compressed(os.path.join(HERE, "g1_tiny.npz"), **out)

    # ---- G2: full 8x256, sampled parameter gradients ---------------------------------------
    out = {}
    hid = [256] * 8
    p32 = synth.siren_params(hid, seed=123, dtype=np.float32)
    b32 = synth.training_batch(192, seed=123, dtype=np.float32)
    n_theta = synth.flatten_params(p32).size
    sample = np.arange(0, n_theta, 61)
    out["hidden"] = np.array(hid); out["sample"] = sample
    out["param_seed"] = np.array(123); out["batch_seed"] = np.array(123); out["n_points"] = np.array(192)
    # fp64 arithmetic on the fp32-representable weights/inputs = the "exact" answer for those inputs
    run_losses(hid, p32, b32, torch.float64, "f64", out, sample)
    run_losses(hid, p32, b32, torch.float32, "f32", out, sample)
    np.savez_compressed(os.path.join(HERE, "g2_8x256.npz"), **out)

    # ---- G3: N-step Adam trajectories --------------------------------------------------------
    out = {}
    hid = [64] * 4
    p32 = synth.siren_params(hid, seed=11, dtype=np.float32)
    for name, mode, w, lr in (("s1eik", "s1", [1e4, 1e4, 0.0, 1e3], 1e-4), ("s2", "s2", [1e5, 1e5], 1e-6),
                              ("s1full", "s1", [1e4, 1e4, 1e4, 1e3], 1e-4)):
        for dt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            hist, theta = trajectory(hid, p32, 384, 20, lr, mode, w, dt, seed=11)
            out[f"{name}_{tag}_hist"] = hist
            out[f"{name}_{tag}_theta"] = theta
    out["hidden"] = np.array(hid); out["param_seed"] = np.array(11); out["batch_seed"] = np.array(11)
    out["n_points"] = np.array(384); out["steps"] = np.array(20)
    np.savez_compressed(os.path.join(HERE, "g3_traj.npz"), **out)

    out = {}
    hid = [256] * 8
    p32 = synth.siren_params(hid, seed=123, dtype=np.float32)
    n_theta = synth.flatten_params(p32).size
    sample = np.arange(0, n_theta, 61)
    for dt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
        hist, theta = trajectory(hid, p32, 1024, 10, 1e-4, "s1", [1e4, 1e4, 0.0, 1e3], dt, seed=123)
        out[f"s1eik_{tag}_hist"] = hist
        out[f"s1eik_{tag}_theta_sample"] = theta[sample]
    out["hidden"] = np.array(hid); out["sample"] = sample; out["param_seed"] = np.array(123)
    out["batch_seed"] = np.array(123); out["n_points"] = np.array(1024); out["steps"] = np.array(10)
    np.savez_compressed(os.path.join(HERE, "g3_traj_8x256.npz"), **out)

    # ---- G4: chunked query through src.evaluate.evaluate on a small grid ----------------------
    out = {}
    hid = [256] * 8
    p32 = synth.siren_params(hid, seed=123, dtype=np.float32)
    model = ref_model(hid, p32, torch.float32)
    n = 12
    ax = np.linspace(-1.0, 1.0, n, dtype=np.float32)
    grid = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    grads = np.zeros((n ** 3, 3)); hess = np.zeros((n ** 3, 3, 3))
    vals = evaluate(model, grid, max_batch=500, device=torch.device("cpu"), gradients=grads, hessians=hess)
    out["grid_n"] = np.array(n); out["values"] = vals; out["gradients"] = grads; out["hessians"] = hess
    out["inv_tanh"] = inverse("tanh", np.abs(vals), 100)
    np.savez_compressed(os.path.join(HERE, "g4_query.npz"), **out)
    # ---- G5: the reference's own example mesh (data/beetle), BASELINE config 0/1 -------------------------------
    # batches from THIS repo's sampler restatement (oracle/sampler_oracle.py) on tests/golden/beetle.obj; the
    # reference's loss_s1 + torch.optim.Adam run on exactly those batches gives the curve to follow.
    from diffudf_amd import mesh
    from oracle import sampler_oracle as SO
    out = {}
    hid = [256] * 8
    p32 = synth.siren_params(hid, seed=123, dtype=np.float32)
    n_theta = synth.flatten_params(p32).size
    sample = np.arange(0, n_theta, 61)
    tri, pos, nrm = mesh.prepare(os.path.join(HERE, "beetle"), 100000, seed=123)
    bs, steps = 3000, 12
    n_on, n_off = int(bs * 0.333), int(bs * 0.666)
    n_far, n_near = n_off // 2, n_off - n_off // 2
    batches = [SO.sample_batch(tri, pos, nrm, n_on, n_far, n_near, seed=123, step=t) for t in range(steps)]
    for name, w in (("s1eik", [1e4, 1e4, 0.0, 1e3]), ("s1full", [1e4, 1e4, 1e4, 1e3])):
        for dt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            model = ref_model(hid, p32, dt)
            opt = torch.optim.Adam(lr=1e-4, params=model.parameters())
            hist = []
            for t in range(steps):
                x, nr, sd = [torch.from_numpy(a.astype(np.float64)).to(dt)[None] for a in batches[t]]
                opt.zero_grad()
                terms = loss_s1(model, x, {"normals": nr, "sdf": sd}, w, 100)
                total = torch.zeros((1, 1), dtype=dt)
                for v in terms.values():
                    total = total + v
                total.backward()
                opt.step()
                hist.append([float(v) for v in terms.values()])
            theta = np.concatenate([p.detach().reshape(-1).double().numpy() for p in model.parameters()])
            out[f"{name}_{tag}_hist"] = np.array(hist)
            out[f"{name}_{tag}_theta_sample"] = theta[sample]
    out["hidden"] = np.array(hid); out["sample"] = sample; out["param_seed"] = np.array(123)
    out["batch_seed"] = np.array(123); out["batch_size"] = np.array(bs); out["steps"] = np.array(steps)
    out["surface_points"] = np.array(100000)
    out["batch0_x"] = batches[0][0]; out["batch0_sdf"] = batches[0][2]
    np.savez_compressed(os.path.join(HERE, "g5_beetle.npz"), **out)
    make_g6()
    make_g7()
    make_g8()
    make_g9()
    print("golden fixtures written to", HERE)


def make_g12():
    """G12 (SURVEY 8(c) G3, N = 50): the trajectory bar at a length where a format's noise has time to grow.
    (a) beetle: 50 Adam steps of the Eikonal `loss_s1` on the sampler oracle's batches (steps 0..49 of the stream g5 uses,
        2997 points), fp64 and fp32 reference runs;
    (b) synthetic 8x256: 40 Eikonal steps at lr 1e-4 followed by 10 `loss_s2` steps at lr 1e-5 (the reference's own s1 -> s2
        schedule, train.py:179-191, shortened), 1024 points per step, fp64 and fp32."""
    from diffudf_amd import mesh
    from oracle import sampler_oracle as SO
    out = {}
    hid = [256] * 8
    p32 = synth.siren_params(hid, seed=123, dtype=np.float32)
    n_theta = synth.flatten_params(p32).size
    sample = np.arange(0, n_theta, 61)
    tri, pos, nrm = mesh.prepare(os.path.join(HERE, "beetle"), 100000, seed=123)
    bs, steps = 3000, 50
    n_on, n_off = int(bs * 0.333), int(bs * 0.666)
    n_far, n_near = n_off // 2, n_off - n_off // 2
    batches = [SO.sample_batch(tri, pos, nrm, n_on, n_far, n_near, seed=123, step=t) for t in range(steps)]
    w = [1e4, 1e4, 0.0, 1e3]
    for dt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
        model = ref_model(hid, p32, dt)
        opt = torch.optim.Adam(lr=1e-4, params=model.parameters())
        hist = []
        for t in range(steps):
            x, nr, sd = [torch.from_numpy(a.astype(np.float64)).to(dt)[None] for a in batches[t]]
            opt.zero_grad()
            terms = loss_s1(model, x, {"normals": nr, "sdf": sd}, w, 100)
            total = torch.zeros((1, 1), dtype=dt)
            for v in terms.values():
                total = total + v
            total.backward()
            opt.step()
            hist.append([float(v) for v in terms.values()])
        theta = np.concatenate([p.detach().reshape(-1).double().numpy() for p in model.parameters()])
        out[f"beetle_s1eik_{tag}_hist"] = np.array(hist)
        out[f"beetle_s1eik_{tag}_theta_sample"] = theta[sample]
    out["beetle_batch_size"] = np.array(bs); out["beetle_steps"] = np.array(steps); out["surface_points"] = np.array(100000)
    # (b) synthetic s1 -> s2 schedule
    n_pts, s1_steps, s2_steps = 1024, 40, 10
    for dt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
        model = ref_model(hid, p32, dt)
        opt = torch.optim.Adam(lr=1e-4, params=model.parameters())
        h1, h2 = [], []
        for t in range(s1_steps + s2_steps):
            x, nr, sd = [torch.from_numpy(a.astype(np.float64)).to(dt)[None]
                         for a in synth.training_batch(n_pts, seed=123, step=t, dtype=np.float64)]
            if t == s1_steps:
                for g in opt.param_groups:                     # train.py:184-191: stage 2 runs at a lower rate
                    g["lr"] = 1e-5
            opt.zero_grad()
            if t < s1_steps:
                terms = loss_s1(model, x, {"normals": nr, "sdf": sd}, w, 100)
            else:
                terms = loss_s2(model, x, {"normals": nr, "sdf": sd}, [1e5, 1e5], 100)
            total = torch.zeros((1, 1), dtype=dt)
            for v in terms.values():
                total = total + v
            total.backward()
            opt.step()
            (h1 if t < s1_steps else h2).append([float(v) for v in terms.values()])
        theta = np.concatenate([p.detach().reshape(-1).double().numpy() for p in model.parameters()])
        out[f"synth_s1_{tag}_hist"] = np.array(h1); out[f"synth_s2_{tag}_hist"] = np.array(h2)
        out[f"synth_{tag}_theta_sample"] = theta[sample]
    out["hidden"] = np.array(hid); out["sample"] = sample; out["param_seed"] = np.array(123); out["batch_seed"] = np.array(123)
    out["synth_n_points"] = np.array(n_pts); out["synth_s1_steps"] = np.array(s1_steps); out["synth_s2_steps"] = np.array(s2_steps)
    np.savez_compressed(os.path.join(HERE, "g12_traj50.npz"), **out)
    print("g12 written")


if __name__ == "__main__":
    if sys.argv[1:] == ["g6"]:
        make_g6()
    elif sys.argv[1:] == ["g7"]:
        make_g7()
    elif sys.argv[1:] == ["g8"]:
        make_g8()
    elif sys.argv[1:] == ["g9"]:
        make_g9()
    elif sys.argv[1:] == ["g10"]:
        make_g10()
    elif sys.argv[1:] == ["g11"]:
        make_g11()
    elif sys.argv[1:] == ["g12"]:
        make_g12()
    elif sys.argv[1:] == ["g13"]:
        make_g13()
    else:
        main()
