#!/usr/bin/env python
# coding: utf-8
"""Generate tests/golden/g14_pointcloud.npz by RUNNING THE REFERENCE ITSELF (same discipline as make_golden.py: the
reference is resolved from its read-only mount, nothing of it is copied; build container only).

    python tests/golden/make_golden_pc.py

Contents, per network `t` (4x128, trained here for a few hundred Adam steps of the reference's loss_s1 on batches of
tests/golden/beetle.obj drawn by this repo's CPU sampler oracle — a random SIREN is not a distance field) and `s` (8x256 from
synth.siren_params(seed 123), shape coverage only), and per gt_mode in ('tanh', 'siren'):
  core : fixed float64 start points (uniform candidates for which the reference's own float32 and float64 runs agree) and the outputs of the reference's inner loop (src/render_pc.py:43-56) re-issued around the
         imported reference `evaluate`, `inverse`, `normalize`: moved samples, last steps, accept mask, pre-move gradients and
         Hessians, normals;
  fate : the same loop with the reference model in float64 — fraction of points whose accept/reject agrees (asserted >= 0.995);
  e2e  : (network `t`, 'tanh') two runs of the reference's own Sampler.generate_point_cloud (CPU, num_points 4096, np.random.seed
         0 and 1), their symmetric mean nearest-neighbour distance d_ref and mean |n.n'| of nearest neighbours c_ref.
"""
import os
import sys
import types
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, "/root/reference")          # `src.*` must resolve to the REFERENCE here, not to this repo's shim
sys.path[:] = [p for p in sys.path if os.path.abspath(p or ".") != REPO] + [REPO]
if not hasattr(np, "bool8"):
    np.bool8 = np.bool_                          # reference src/render_pc.py:55 on a current numpy (this process only)
if "tqdm" not in sys.modules:
    try:
        import tqdm  # noqa: F401
    except ImportError:
        sys.modules["tqdm"] = types.SimpleNamespace(tqdm=lambda it, *a, **k: it)

from src.model import SIREN                                     # noqa: E402  (reference)
from src.evaluate import evaluate                               # noqa: E402  (reference)
from src.inverses import inverse                                # noqa: E402  (reference)
from src.util import normalize                                  # noqa: E402  (reference)
from src.loss_functions import loss_s1                          # noqa: E402  (reference)
from src.render_pc import Sampler                               # noqa: E402  (reference)
from diffudf_amd import synth, mesh                             # noqa: E402
from oracle import sampler_oracle                               # noqa: E402

torch.set_num_threads(8)
CPU = torch.device("cpu")
ALPHA, THRESH, STEPS = 100.0, 0.01, 5
HID_T, HID_S = [128] * 4, [256] * 8


def model_from(hidden, params, dtype=torch.float32):
    m = SIREN(3, 1, hidden, w0=30).double()
    sd = {}
    for i, (w, b) in enumerate(params):
        sd[f"net.{i}.0.weight"] = torch.from_numpy(np.asarray(w, dtype=np.float64))
        sd[f"net.{i}.0.bias"] = torch.from_numpy(np.asarray(b, dtype=np.float64))
    m.load_state_dict(sd)
    return m.to(dtype).eval()


def train_small(steps=400, seed=7):
    verts, tris = mesh.load_obj(os.path.join(HERE, "beetle.obj"))
    verts = mesh.normalize_vertices(verts)
    pc_pos, pc_nrm = mesh.sample_surface(verts, tris, 20000, seed=seed)
    tri = mesh.triangle_soup(verts, tris)
    torch.manual_seed(seed)
    m = SIREN(3, 1, HID_T, w0=30)
    opt = torch.optim.Adam(m.parameters(), lr=1e-4)
    w = [1e4, 1e4, 0.0, 1e3]
    for step in range(steps):
        x, nrm, sdf = sampler_oracle.sample_batch(tri, pc_pos, pc_nrm, 400, 400, 400, seed, step)
        gt = {"sdf": torch.from_numpy(sdf)[None], "normals": torch.from_numpy(nrm)[None]}
        terms = loss_s1(m, torch.from_numpy(x)[None], gt, w, ALPHA)
        loss = sum(t for t in terms.values())
        opt.zero_grad(); loss.backward(); opt.step()
        if step % 100 == 0 or step + 1 == steps:
            print(f"  train step {step}: loss {float(loss.detach()):.4f}")
    return [(l[0].weight.detach().numpy().copy(), l[0].bias.detach().numpy().copy()) for l in m.net]


def inner_loop(model, start, gt_mode):
    """reference src/render_pc.py:41-56, line by line, around the imported reference functions"""
    samples = start.copy()
    n = len(samples)
    f64 = next(model.parameters()).dtype == torch.float64
    feed = (lambda a: torch.from_numpy(a)) if f64 else (lambda a: a)      # evaluate() casts numpy input to float32 (:18); a float64 model takes the tensor
    gradients = np.zeros((n, 3))
    pre = None
    with np.errstate(invalid="ignore", divide="ignore"):
        for step in range(STEPS):
            if step == STEPS - 1:
                hessians = np.zeros((n, 3, 3))
                pre = samples.copy()
                udfs = evaluate(model, feed(samples), gradients=gradients, hessians=hessians, device=CPU)
            else:
                udfs = evaluate(model, feed(samples), gradients=gradients, device=CPU)
            steps = inverse(gt_mode, udfs, ALPHA, min_step=0)
            samples -= steps * normalize(gradients)
        dom = np.prod(np.logical_and(samples >= -1, samples <= 1), axis=1).astype(np.bool_)
        acc = (steps.flatten() < THRESH) * dom
    if gt_mode == "siren":
        nrm = normalize(gradients)
    else:
        nrm = np.full((n, 3), np.nan)          # the reference runs eigh on accepted rows only (:65); NaN rows have no frame
    lam = np.full((n, 3), np.nan)
    for i in np.flatnonzero(np.isfinite(hessians).all(axis=(1, 2))):
        w, v = np.linalg.eigh(hessians[i])
        lam[i] = w
        if gt_mode != "siren":
            nrm[i] = v[:, 2]
    return dict(moved=samples, last=steps.flatten(), accept=acc, grad=gradients.copy(), hess=hessians, normals=nrm, lam=lam,
                pre=pre, udf=udfs.flatten())


def cloud_stats(p0, n0, p1, n1):
    def nn(a, b):
        idx = np.empty(len(a), np.int64); d = np.empty(len(a))
        for i in range(0, len(a), 512):
            dd = ((a[i:i + 512, None, :] - b[None]) ** 2).sum(-1)
            idx[i:i + 512] = dd.argmin(1); d[i:i + 512] = np.sqrt(dd.min(1))
        return idx, d
    i01, d01 = nn(p0, p1); i10, d10 = nn(p1, p0)
    d = 0.5 * (d01.mean() + d10.mean())
    c = 0.5 * (np.abs((n0 * n1[i01]).sum(1)).mean() + np.abs((n1 * n0[i10]).sum(1)).mean())
    return float(d), float(c)


def main():
    out = {}
    print("training the 4x128 network")
    nets = {"t": (HID_T, train_small()), "s": (HID_S, synth.siren_params(HID_S, seed=123))}
    n_core = 1500
    for tag, (hidden, params) in nets.items():
        m32, m64 = model_from(hidden, params), model_from(hidden, params, torch.float64)
        if tag == "t":
            out["t_theta"] = synth.flatten_params(params)
        # Candidates: uniform in the box.  Far from the surface the projection is ill-conditioned (steps of the size of the field
        # value through a rough far field): the reference's OWN float32 and float64 runs end up to 7e-3 apart there, while the GPU
        # test holds moved positions to 1e-4.  So, as for the fate margin, the start points are chosen such that the reference
        # alone meets the bound with room to spare: a candidate stays when its float32 and float64 reference runs agree on NaN /
        # accept and end within 2.5e-5 of each other in both modes.  Nothing of the code under test enters the choice.
        cand = np.stack([synth.uniform01(2024, 50 + k, 0, 2 * n_core) * 2.0 - 1.0 for k in range(3)], 1)
        stable = np.ones(len(cand), bool)
        for mode in ("tanh", "siren"):
            r, r64 = inner_loop(m32, cand, mode), inner_loop(m64, cand, mode)
            nan32, nan64 = np.isnan(r["moved"]).any(1), np.isnan(r64["moved"]).any(1)
            with np.errstate(invalid="ignore"):
                close = np.abs(r["moved"] - r64["moved"]).max(1) <= 2.5e-5
            stable &= (nan32 == nan64) & (nan32 | close) & (r["accept"] == r64["accept"])
        print(f"net {tag}: {int(stable.sum())} of {len(cand)} candidates are stable under the reference's own precision")
        assert stable.sum() >= n_core
        start = cand[stable][:n_core].copy()
        out[f"{tag}_start"] = start
        # a few start points chosen where udf < 0 ('tanh': NaN step, rejected)
        u0 = evaluate(m32, start, device=CPU).flatten()
        print(f"net {tag}: {int((u0 < 0).sum())} of {n_core} start points have udf < 0")
        for mode in ("tanh", "siren"):
            r = inner_loop(m32, start, mode)
            r64 = inner_loop(m64, start, mode)
            fate = float((r["accept"] == r64["accept"]).mean())
            with np.errstate(invalid="ignore"):
                sep = (r["lam"][:, 2] - r["lam"][:, 1]) > 1e-2 * np.abs(r["lam"]).max(1)
            acc = r["accept"]
            print(f"  {mode}: accepted {int(acc.sum())}, fate agreement f32/f64 {fate:.4f}, NaN rows {int(np.isnan(r['moved']).any(1).sum())}, "
                  f"accepted with separated top eigenvalues {int((sep & acc).sum())} ({1 - (sep & acc).sum() / max(acc.sum(), 1):.3%} left out)")
            assert fate >= 0.995, (tag, mode, fate)
            if tag == "t" and mode == "tanh":
                assert 1 - (sep & acc).sum() / max(acc.sum(), 1) < 0.05
            k = f"{tag}_{mode}_"
            out[k + "moved"] = r["moved"]; out[k + "last"] = r["last"]; out[k + "accept"] = acc
            out[k + "grad"] = r["grad"].astype(np.float32); out[k + "hess"] = r["hess"].astype(np.float32)
            out[k + "normals"] = r["normals"].astype(np.float32); out[k + "fate"] = np.float64(fate)
            out[k + "udf"] = r["udf"].astype(np.float32)
    # end to end: the reference's own Sampler on the trained network
    hidden, params = nets["t"]
    import tempfile
    ckpt = os.path.join(tempfile.mkdtemp(), "g14_ckpt.pth")
    torch.save(model_from(hidden, params).state_dict(), ckpt)
    clouds = []
    for seed in (0, 1):
        np.random.seed(seed)
        s = Sampler(3, hidden, 30, None, ckpt, "cpu")
        import warnings
        with warnings.catch_warnings(), np.errstate(invalid="ignore", divide="ignore"):
            warnings.simplefilter("ignore")
            p, nr = s.generate_point_cloud("tanh", ALPHA, STEPS, 4096, THRESH, 200)
        print(f"  e2e seed {seed}: {len(p)} points")
        assert len(p) >= 4096
        clouds.append((p, nr))
    os.remove(ckpt)
    d_ref, c_ref = cloud_stats(clouds[0][0], clouds[0][1], clouds[1][0], clouds[1][1])
    print(f"  d_ref {d_ref:.5f}  c_ref {c_ref:.4f}")
    out["e2e_points0"] = clouds[0][0].astype(np.float32); out["e2e_normals0"] = clouds[0][1].astype(np.float32)
    out["e2e_d_ref"] = np.float64(d_ref); out["e2e_c_ref"] = np.float64(c_ref)
    out["alpha"] = np.float64(ALPHA); out["surf_thresh"] = np.float64(THRESH); out["num_steps"] = np.int64(STEPS)
    path = os.path.join(HERE, "g14_pointcloud.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
