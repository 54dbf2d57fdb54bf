# coding: utf-8
"""GPU: `generate_st` with gt_mode 'gt' (configs/st_beetle_gt.json) — the sphere-traced image of the ground-truth mesh — against
the same image composed in numpy from `MeshIndex` calls."""
import json
import os

import numpy as np
import pytest
import torch

import mesh_occupancy_oracle as OO
from diffudf_amd import hip_ops, render_st

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def numpy_image(scene, rc, noise):
    """Reference src/render_st.py:255-281 in numpy around `MeshIndex.distance` / `.signed_distance`, shading as that code means it:
    Blinn-Phong without a specular term (grey 0.7 diffuse, 0.2 ambient, clipped to [0, 0.9]); background 1."""
    import generate_st
    n = rc["height"]
    rays, t0, mask = hip_ops.render_setup_rays(n, rc["width"], rc["fov"], noise, generate_st.camera_rotation(rc["camera_position"]),
                                               rc["camera_position"], [1, -1, 1, -1, 1, -1], DEV)
    rays, t0, mask = rays.cpu().numpy(), t0.cpu().numpy(), mask.cpu().numpy().astype(bool)
    hits, fragile = OO.march(lambda p: scene.distance(dev(p)).cpu().numpy(), rays, t0, mask, rc["surface_threshold"], rc["max_iterations"])
    sd = lambda p: scene.signed_distance(dev(p.astype(np.float32))).cpu().numpy()          # noqa: E731
    P, k, eps = t0[hits], int(hits.sum()), 0.0001
    grad = np.vstack([(sd(P + np.tile(np.eye(1, 3, i), (k, 1)) * eps) - sd(P - np.tile(np.eye(1, 3, i), (k, 1)) * eps)) / (2 * eps)
                      for i in range(3)]).T
    assert grad.dtype == np.float32
    normals = grad / np.linalg.norm(grad, axis=1, keepdims=True)
    normals = normals * np.where(np.sum(normals * rays[hits], axis=1, keepdims=True) > 0, -1.0, 1.0)
    to_light = np.asarray(rc["light_position"], dtype=np.float64)[None, :] - P
    to_light /= np.linalg.norm(to_light, axis=1, keepdims=True)
    lambertian = np.maximum(np.sum(normals * to_light, axis=1, keepdims=True), 0.0)
    colors = np.ones_like(t0)
    colors[hits] = np.clip(0.7 * lambertian + 0.2, 0, 0.9)
    return (colors / 1 * 255).astype(np.uint8).reshape(n, rc["width"], 3), hits, fragile


def test_generate_st_renders_the_mesh():
    import generate_st
    with open(os.path.join(REPO, "configs", "st_beetle_gt.json")) as f:
        cfg = json.load(f)
    assert cfg["network_config"]["gt_mode"] == "gt" and cfg["network_config"]["mesh_path"] == "tests/golden/beetle"
    cfg["rendering_config"].update(width=32, height=32, sample_rate=1)
    np.random.seed(7)
    im = np.asarray(generate_st.generate_st(cfg))
    assert im.shape == (32, 32, 3) and im.dtype == np.uint8
    np.random.seed(7)
    noise = np.random.normal(0.5, 0.35)
    scene = render_st.load_scene(os.path.join(REPO, cfg["network_config"]["mesh_path"]), DEV)
    want, hits, fragile = numpy_image(scene, cfg["rendering_config"], noise)
    background = (im == 255).all(axis=2).reshape(-1)
    print(f"generate_st gt: {int(hits.sum())} hit pixels, {int(background.sum())} background, {int(fragile.sum())} fragile rays, "
          f"max grey difference {int(np.abs(im.astype(int) - want.astype(int)).max())}")
    assert 0 < hits.sum() < 1024 and np.array_equal(background, ~hits)                 # hit and background pixels
    assert (im.reshape(-1, 3)[hits] <= 230).all() and (im.reshape(-1, 3)[hits] >= 50).all()      # 0.2 .. 0.9 of 255
    assert np.abs(im.astype(int) - want.astype(int)).max() <= 1
    cfg["rendering_config"]["specular"] = True                                          # shininess 40: highlights only brighten
    np.random.seed(7)
    spec = np.asarray(generate_st.generate_st(cfg))
    print("specular: pixels brightened", int((spec > im).any(axis=2).sum()))
    assert spec.shape == im.shape and (spec >= im).all()
