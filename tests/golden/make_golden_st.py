#!/usr/bin/env python
# coding: utf-8
"""Generate tests/golden/g15_render.npz by RUNNING THE REFERENCE ITSELF (same discipline as make_golden_pc.py: the reference is
resolved from its read-only mount, nothing of it is copied; build container only).

    python tests/golden/make_golden_st.py

The network is the trained 4x128 one of g14_pointcloud.npz (`t_theta`).  Every scene is one call of the reference's own
`generate_st(config)` on the CPU (temporary checkpoint, np.random.seed(SEED) so that all scenes draw the same jitter), with
recorders wrapped around `create_projectional_image`, `compute_normals_and_cd`, `compute_curvature`, `np.percentile`,
`phong_shading` and `ward_reflectance` in the reference modules' namespaces (this process only).  Images are SIZE x SIZE (square:
the reference swaps width and height when it calls get_pixels_camera), sample_rate 2.

  a : oblique camera of the reference's config, 'tanh', blinn-phong (shininess 20), plot_curvatures 'mean'
  b : the same camera, ward with alpha1 = alpha2, 'gaussian'
  c : camera on the +z axis (rotation branch a@b = 1: the identity), 'tanh', no curvature, shininess 40, gd_steps 3
  d : the oblique camera, scene c's settings with gt_mode 'siren' (gradient normals, `udfs < threshold` hit test)
  e : camera on the -z axis (branch a@b = -1), fov 120 so that part of the rays miss the box: ray set-up only, the run stops after the first pass's arguments are recorded

Stored (PASS 0 of each scene unless said otherwise; the file has to stay below 1 MiB, so whatever a test can rebuild exactly is
stored in its smallest form — hit rows only, colour-map output as table rows, grey images as one channel):
  jitter (2), lut (256,3) the table the reference used, pixels_x / pixels_y (get_pixels_camera of pass 0: its first row of x, its
  first column of y; z = -1),
  obl_* / pz_* : rays, t0, mask handed to create_projectional_image (a, b, d share obl_*: same seed, same camera); nz_* for e
  (rays and t0 of every 8th ray, the whole mask);  b shares a's hits, positions, mask and normals (asserted equal, stored once)
  {s}_hits, {s}_pos = t0[hits] after marching and descent, {s}_mask_after, {s}_img = returned image at the hit pixels
  a, b: {s}_normals_raw / {s}_pcd / {s}_curv_raw as the eigensolver / compute_curvature returned them (float32), {s}_normals,
        {s}_curv = oriented (what the percentiles saw), {s}_bounds, {s}_cmap_rows (row of `lut` of every hit)
  a_final : the uint8 image of both passes;   wardx_img : ward_reflectance re-run on b's hits with alpha1 != alpha2
  syn_* : six synthetic hits whose Ward weight is NaN, +inf and -inf, through the reference's function
  {s}_fate, {s}_coldiff_p50, {s}_coldiff_p99 : pass 0 re-issued through the reference's create_projectional_image around the
        reference model in float64 (the reference's `evaluate` casts numpy input to float32, so the double model sits behind a
        cast) — share of pixels whose hit / miss agrees, and median / 99th percentile of the per-channel colour difference on pixels
        that hit in both.  fate >= 0.99 is asserted.
"""
import importlib.util
import json
import os
import sys
import tempfile
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, REF)                        # `src.*` must resolve to the REFERENCE here, not to this repo's shim
sys.path[:] = [p for p in sys.path if os.path.abspath(p or ".") != REPO] + [REPO]
if not hasattr(np, "bool8"):
    np.bool8 = np.bool_                        # reference src/render_st.py:137 on a current numpy (this process only)
if "open3d" not in sys.modules:                # reference src/render_st.py:8-9 imports it at module level; only the gt renderer uses it
    o3d = types.ModuleType("open3d"); o3d.core = types.ModuleType("open3d.core")
    sys.modules["open3d"] = o3d; sys.modules["open3d.core"] = o3d.core
import matplotlib                              # noqa: E402
import matplotlib.cm                           # noqa: E402
if not hasattr(matplotlib.cm, "get_cmap"):
    matplotlib.cm.get_cmap = matplotlib.colormaps.get_cmap          # reference src/render_st.py:89 on matplotlib >= 3.9

from src.model import SIREN                    # noqa: E402  (reference)
import src.render_st as ref_rs                 # noqa: E402  (reference)
spec = importlib.util.spec_from_file_location("ref_generate_st", os.path.join(REF, "generate_st.py"))
ref_gs = importlib.util.module_from_spec(spec); spec.loader.exec_module(ref_gs)      # the reference's script



class _Chunks(list):
    """reference src/render_st.py:82 calls `.squeeze(0)` on the LIST its `evaluate` returns (the 'siren' branch cannot run as it
    stands; the value is not used afterwards).  The list handed out here answers that call — this process only."""

    def squeeze(self, *a):
        return torch.hstack(list(self)).squeeze(*a)


_ref_evaluate = ref_rs.evaluate
ref_rs.evaluate = lambda *a, **k: (lambda r: (r[0], _Chunks(r[1])))(_ref_evaluate(*a, **k))

torch.set_num_threads(8)
CPU = torch.device("cpu")
SIZE, SEED, HID, NZ_STRIDE = 64, 15, [128] * 4, 8
OBLIQUE, PLUS_Z, MINUS_Z = [0.8939, 0.7, 2.86], [0, 0, 2.9], [0, 0, -2.9]


def config(ckpt, camera, gt_mode="tanh", method="blinn-phong", plot="none", shininess=20, gd_steps=0, fov=45):
    return {"network_config": {"alpha": 100, "device": "cpu", "gt_mode": gt_mode, "hidden_layer_nodes": HID, "w0": 30, "model_path": ckpt},
            "rendering_config": {"width": SIZE, "height": SIZE, "surface_threshold": 0.004, "fov": fov, "camera_position": camera,
                                 "light_position": [1, 2.38206, 10], "plot_curvatures": plot, "max_iterations": 100,
                                 "reflection_method": method, "curv_low_bound": 5, "curv_high_bound": 95, "alpha1": 0.2, "alpha2": 0.2,
                                 "shininess": shininess, "sample_rate": 2, "gd_steps": gd_steps, "rotation": 0, "output_path": ""}}


SCENES = {"a": dict(camera=OBLIQUE, plot="mean"), "b": dict(camera=OBLIQUE, method="ward", plot="gaussian"),
          "c": dict(camera=PLUS_Z, shininess=40, gd_steps=3), "d": dict(camera=OBLIQUE, gt_mode="siren", shininess=40, gd_steps=3),
          "e": dict(camera=MINUS_Z, fov=120)}


class Stop(Exception):
    pass


class Recorder:
    """Wraps the reference's functions in ITS modules' namespaces and keeps what went through them, per pass."""

    def __init__(self):
        self.real = {n: getattr(ref_rs, n) for n in ("compute_normals_and_cd", "compute_curvature", "phong_shading", "ward_reflectance")}
        self.real_cpi, self.real_np, self.real_gpc = ref_gs.create_projectional_image, ref_rs.np, ref_gs.get_pixels_camera
        self.passes, self.stop_after_setup = [], False
        rec = self

        class NumpyProxy:                                  # `np` of reference src/render_st.py: percentile records, the rest passes through
            def __getattr__(self, name):
                return getattr(rec.real_np, name)

            def percentile(self, a, q, *args, **kw):
                out = rec.real_np.percentile(a, q, *args, **kw)
                rec.cur.setdefault("curv", np.array(a, copy=True)); rec.cur.setdefault("bounds", []).append(out)
                return out
        ref_rs.np = NumpyProxy()
        ref_rs.compute_normals_and_cd = self.frames
        ref_rs.compute_curvature = self.curvature
        ref_rs.phong_shading = lambda *a, **k: self.shade("phong_shading", a, k)
        ref_rs.ward_reflectance = lambda *a, **k: self.shade("ward_reflectance", a, k)
        ref_gs.create_projectional_image = self.cpi
        ref_gs.get_pixels_camera = self.pixels

    def restore(self):
        for n, f in self.real.items():
            setattr(ref_rs, n, f)
        ref_rs.np = self.real_np
        ref_gs.create_projectional_image, ref_gs.get_pixels_camera = self.real_cpi, self.real_gpc

    def pixels(self, width, height, fov, noise):
        self.pending = dict(jitter=float(noise), pixels=self.real_gpc(width, height, fov, noise))
        return self.pending["pixels"]

    def cpi(self, model, rays, t0, mask_rays, network_config, rendering_config, device):
        self.cur = dict(self.pending, rays=rays.copy(), t0=t0.copy(), mask=mask_rays.copy(), normals_raw=[], pcd=[], curv_raw=[])
        self.passes.append(self.cur)
        if self.stop_after_setup:
            raise Stop()
        img = self.real_cpi(model, rays=rays, t0=t0, mask_rays=mask_rays, network_config=network_config,
                            rendering_config=rendering_config, device=device)
        self.cur.update(t0_after=t0.copy(), mask_after=mask_rays.copy(), image=img.copy())
        return img

    def frames(self, inputs, outputs):
        n, pcd = self.real["compute_normals_and_cd"](inputs, outputs)
        self.cur["normals_raw"].append(n.detach().squeeze(0).numpy().copy()); self.cur["pcd"].append(pcd.squeeze(0).numpy().copy())
        return n, pcd

    def curvature(self, inputs, normals, **kw):
        c = self.real["compute_curvature"](inputs, normals, **kw)
        self.cur["curv_raw"].append(c.numpy().reshape(-1).copy())
        return c

    def shade(self, name, a, k):
        names = {"phong_shading": ("light_position", "shininess", "hits", "samples", "normals", "color_map"),
                 "ward_reflectance": ("light_position", "camera_position", "hits", "samples", "normals", "alpha1", "alpha2", "pc1", "pc2",
                                      "color_map")}[name]
        args = dict(zip(names, a)); args.update(k)
        self.cur["shade"] = {n: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for n, v in args.items()}
        self.cur["shade_fn"] = name
        return self.real[name](*a, **k)


class Behind32(torch.nn.Module):
    """The reference model in float64 behind the float32 cast of the reference's `evaluate` (src/render_st.py:25)."""

    def __init__(self, m64):
        super().__init__()
        self.m64 = m64

    def forward(self, x):
        return self.m64(x.double())


def state_dict_of(theta):
    sd, o, n_in = {}, 0, 3
    for i, h in enumerate(HID + [1]):
        sd[f"net.{i}.0.weight"] = torch.from_numpy(theta[o:o + h * n_in].reshape(h, n_in).copy()); o += h * n_in
        sd[f"net.{i}.0.bias"] = torch.from_numpy(theta[o:o + h].copy()); o += h
        n_in = h
    assert o == theta.size
    return sd


def run_scene(cfg, setup_only=False):
    rec = Recorder(); rec.stop_after_setup = setup_only
    np.random.seed(SEED)
    try:
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            im = ref_gs.generate_st(cfg)
    except Stop:
        im = None
    finally:
        rec.restore()
    return rec.passes, (None if im is None else np.asarray(im))


def main():
    theta = np.load(os.path.join(HERE, "g14_pointcloud.npz"))["t_theta"].astype(np.float32)
    sd = state_dict_of(theta)
    ckpt = os.path.join(tempfile.mkdtemp(), "g15_ckpt.pth")
    torch.save(sd, ckpt)
    m64 = SIREN(n_in_features=3, n_out_features=1, hidden_layer_config=HID, w0=30, ww=None).double()
    m64.load_state_dict({k: v.double() for k, v in sd.items()})
    cmap = matplotlib.colormaps['RdYlBu']
    lut = np.ascontiguousarray(cmap(np.arange(cmap.N))[:, :3])
    out = {"lut": lut, "size": np.int64(SIZE), "seed": np.int64(SEED)}
    for tag, kw in SCENES.items():
        cfg = config(ckpt, **kw)
        passes, final = run_scene(cfg, setup_only=(tag == "e"))
        p0 = passes[0]
        out.setdefault("jitter", np.array([p["jitter"] for p in passes]))
        if "pixels_x" not in out:                        # separable: one row of x and one column of y say it all
            px = p0["pixels"]
            assert np.array_equal(px[..., 0], np.tile(px[0, :, 0], (SIZE, 1))) and np.array_equal(px[..., 1], np.tile(px[:, 0, 1][:, None], (1, SIZE)))
            assert np.all(px[..., 2] == -1)
            out["pixels_x"], out["pixels_y"] = px[0, :, 0].copy(), px[:, 0, 1].copy()
        cam = {"a": "obl", "c": "pz", "e": "nz"}.get(tag)
        if cam:
            sub = slice(None, None, NZ_STRIDE) if tag == "e" else slice(None)       # e: every NZ_STRIDE-th ray (file size)
            out[cam + "_rays"], out[cam + "_t0"], out[cam + "_mask"] = p0["rays"][sub], p0["t0"][sub], p0["mask"]
            print(f"camera {cam}: {int(p0['mask'].sum())} of {len(p0['mask'])} rays enter the box")
            if tag == "e":
                out["nz_fov"] = np.float64(cfg["rendering_config"]["fov"])
                assert 0 < p0["mask"].sum() < len(p0["mask"]) and not p0["mask"][::NZ_STRIDE].all()
        else:
            assert np.array_equal(p0["rays"], out["obl_rays"]) and np.array_equal(p0["t0"], out["obl_t0"])
        if tag == "b":                                   # a and b march alike: b's hits, positions and frames are a's (not stored twice)
            assert np.array_equal(p0["shade"]["hits"], out["a_hits"]) and np.array_equal(p0["t0_after"][out["a_hits"]], out["a_pos"])
            assert np.array_equal(np.concatenate(p0["normals_raw"]), out["a_normals_raw"])
            assert np.array_equal(p0["shade"]["normals"], out["a_normals"]) and np.array_equal(p0["mask_after"], out["a_mask_after"])
        if tag == "e":
            continue
        assert np.allclose(out["jitter"], [p["jitter"] for p in passes])
        sh = p0["shade"]; hits = sh["hits"]; k = int(hits.sum())
        img = p0["image"].reshape(-1, 3)
        assert np.all(img[~hits] == 1.0)
        if tag != "b":
            out[f"{tag}_hits"] = hits; out[f"{tag}_mask_after"] = p0["mask_after"]; out[f"{tag}_pos"] = p0["t0_after"][hits]
        grey = kw.get("plot", "none") == "none"
        if grey:
            assert np.array_equal(img[:, 0], img[:, 1]) and np.array_equal(img[:, 0], img[:, 2])
        out[f"{tag}_img"] = img[hits][:, 0] if grey else img[hits]
        out[f"{tag}_config"] = np.array(json.dumps({**cfg["rendering_config"], "gt_mode": cfg["network_config"]["gt_mode"]}))
        if tag in ("a", "b"):
            raw_n, pcd, raw_c = np.concatenate(p0["normals_raw"]), np.concatenate(p0["pcd"]), np.concatenate(p0["curv_raw"])
            assert raw_n.dtype == np.float32 and pcd.dtype == np.float32 and raw_c.dtype == np.float32 and len(raw_n) == k
            out[f"{tag}_curv_raw"] = raw_c
            if tag == "a":
                out["a_normals_raw"] = raw_n
                out["a_normals"] = sh["normals"].astype(np.float32); assert np.array_equal(out["a_normals"], sh["normals"])
            out[f"{tag}_curv"] = p0["curv"].reshape(-1); out[f"{tag}_bounds"] = np.array(p0["bounds"], dtype=np.float32)
            rows = np.array([np.flatnonzero((lut == c).all(1))[0] for c in sh["color_map"]], dtype=np.uint8)
            assert np.array_equal(lut[rows], sh["color_map"])
            out[f"{tag}_cmap_rows"] = rows
            if tag == "b":
                out["b_pcd"] = pcd
                assert np.array_equal(pcd[..., 0], sh["pc1"]) and np.array_equal(pcd[..., 1], sh["pc2"])
                with np.errstate(all="ignore"):
                    pos, n = p0["t0_after"][hits], sh["normals"]
                    nl = (n * ref_rs.normalize(np.array(sh["light_position"]) - pos)).sum(1)
                    nv = (n * ref_rs.normalize(np.array(sh["camera_position"]) - pos)).sum(1)
                    print(f"  b: Ward weight NaN on {int((nl * nv < 0).sum())} of {k} hits, infinite on {int((nl * nv == 0).sum())}")
                    assert (nl * nv < 0).sum() > 0
                    wx = ref_rs.ward_reflectance(sh["light_position"], sh["camera_position"], hits, p0["t0_after"], sh["normals"], 0.15, 0.4,
                                                 sh["pc1"], sh["pc2"], color_map=sh["color_map"])
                out["wardx_img"] = wx[hits]; out["wardx_alphas"] = np.array([0.15, 0.4])
        if tag == "a":
            out["a_final"] = final
        # the same pass around the reference model in float64
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            t64, mk64 = p0["t0"].copy(), p0["mask"].copy()
            img64 = ref_rs.create_projectional_image(Behind32(m64), p0["rays"].copy(), t64, mk64, cfg["network_config"],
                                                     cfg["rendering_config"], CPU).reshape(-1, 3)
        hit64 = ~(img64 == 1.0).all(1)
        fate = float((hit64 == hits).mean())
        both = hit64 & hits
        diff = np.abs(img64[both] - img[both]).reshape(-1)
        p50, p99 = float(np.percentile(diff, 50)), float(np.percentile(diff, 99))
        print(f"scene {tag}: {k} hits of {len(hits)} pixels; float32 vs float64: fate {fate:.5f}, colour difference p50 {p50:.3e} p99 {p99:.3e}")
        assert fate >= 0.99, (tag, fate)
        out[f"{tag}_fate"], out[f"{tag}_coldiff_p50"], out[f"{tag}_coldiff_p99"] = np.float64(fate), np.float64(p50), np.float64(p99)
    # synthetic Ward rows: n.l = 0 with n.v > 0 (+inf), n.l = 0 with n.v < 0 (-inf: sqrt(-0.0) = -0.0), n.l * n.v < 0 (NaN)
    light, camera = [0.0, 0.0, 10.0], [0.0, 3.0, 0.5]
    pos = np.array([[0, 0, .5]] * 6, dtype=np.float64)
    n = np.array([[0, 1, 0], [0, -1, 0], [1, 0, 0], [0, 0.6, -0.8], [0, -0.6, 0.8], [0, 0.6, 0.8]], dtype=np.float64)
    pc1 = np.array([[1, 0, 0]] * 6, dtype=np.float64); pc2 = np.cross(n, pc1)
    col = lut[[0, 40, 80, 120, 200, 255]]
    with np.errstate(all="ignore"):
        simg = ref_rs.ward_reflectance(light, camera, np.ones(6, bool), pos, n, 0.2, 0.3, pc1, pc2, color_map=col)
        nl = (n * ref_rs.normalize(np.array(light) - pos)).sum(1); nv = (n * ref_rs.normalize(np.array(camera) - pos)).sum(1)
        w = 1 / np.sqrt(nl * nv)
    print("synthetic Ward weights:", w)
    assert np.isposinf(w).any() and np.isneginf(w).any() and np.isnan(w).any()
    out.update(syn_light=np.array(light), syn_camera=np.array(camera), syn_pos=pos, syn_normals=n, syn_pc1=pc1, syn_pc2=pc2, syn_cmap=col,
               syn_img=simg, syn_alphas=np.array([0.2, 0.3]))
    os.remove(ckpt)
    path = os.path.join(HERE, "g15_render.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
