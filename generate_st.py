#!/usr/bin/env python
# coding: utf-8
"""Sphere-traced image of a trained network — reference generate_st.py:9-156.

    python generate_st.py <config.json>     keys as the reference's configs/st_cfg.json: "network_config" (alpha, device, gt_mode,
                                            hidden_layer_nodes, w0, model_path, + optional "ww") and "rendering_config" (width, height,
                                            fov, camera_position, light_position, surface_threshold, max_iterations, gd_steps,
                                            plot_curvatures 'none' | 'mean' | 'gaussian', curv_low_bound, curv_high_bound,
                                            reflection_method 'blinn-phong' | 'ward', shininess, alpha1, alpha2, sample_rate, rotation,
                                            output_path, + optional "planes")

Every pass — camera rays against the box, marching, the queries at the hits, orientation, curvature colours, the reflection model,
the scatter into the image — and the average over `sample_rate` jittered passes run on the device on ONE accumulator
(`hip_ops.render_pass`); the host reads the hit count of each pass and, at the end, the 8-bit image.

`generate_st` returns a PIL image as the reference does when PIL is importable, otherwise the (H,W,3) uint8 array (written as PNG
through zlib; `rotation != 0` needs PIL and is refused without it).  `render` is the array-level entry.  Like the reference, the
script hands (height, width) to `get_pixels_camera(width, height, ...)` and reshapes by (height, width): images are meant to be
square, and only square images are tested.

gt_mode 'gt' renders the ground-truth MESH instead of a network (reference generate_st.py:103-114, src/render_st.py:248-281):
"network_config" then holds gt_mode, device and "mesh_path" (an OBJ, or a prefix as the training configs give it: `<prefix>_t.obj`,
else `<prefix>.obj` normalised), "rendering_config" the keys above it needs — width, height, fov, camera_position, light_position,
surface_threshold, max_iterations, sample_rate, rotation, output_path, + optional "specular" (Blinn-Phong shininess 40 instead of 0)
and "planes" (`configs/st_beetle_gt.json`).  The march against the mesh is one kernel per pass (`MeshIndex.trace_rays`)."""
import argparse
import json
import os
import struct
import zlib

import numpy as np
import torch

from src.model import SIREN
from src.render_st import (create_projectional_image, create_projectional_image_gt, create_projectional_image_mesh,  # noqa: F401
                           default_colormap, load_scene, mesh_pass)
from diffudf_amd import hip_ops
from diffudf_amd._lib import DudfError


def get_pixels_camera(width, height, fov, noise):
    """(height, width, 3) float64 pixel positions on the z = -1 plane of the camera frame, jittered by `noise` pixels — reference
    generate_st.py:9-33 (host numpy: a public function of that script; the device path forms the same values per pixel)."""
    half = np.tan((fov * np.pi / 180) / 2)
    xs = (2 * ((np.arange(0, width) + noise) / width) - 1) * (width / height) * half
    ys = (2 * ((np.arange(0, height) + noise) / height) - 1) * half
    gx, gy = np.meshgrid(xs, ys, indexing='xy')
    return np.stack([gx, gy, -np.ones_like(gx)], axis=-1)


def camera_rotation(camera_position):
    """The 3x3 that turns the camera frame (looking down -z) towards the origin — reference generate_st.py:44-61: the position as
    float32, b = -position / |position|; b = +z or -z are the two special cases, otherwise columns (right, up, b) with up = e_y
    made orthogonal to b."""
    b = -1 * np.float32(camera_position)
    b /= np.linalg.norm(b)
    c = np.array([0, 0, -1]) @ b
    if np.isclose(c, -1):
        return np.array([[-1.0, 0, 0], [0, 1, 0], [0, 0, -1]])
    if np.isclose(c, 1):
        return np.eye(3)
    e_y = np.array([0, 1, 0])
    up = e_y - (e_y @ b) * b
    up /= np.linalg.norm(up)
    return np.vstack([np.cross(up, b), up, b]).T


def _load_model(network_config):
    dev = network_config["device"]
    dev = torch.device("cuda", dev) if isinstance(dev, int) else torch.device(dev)
    if dev.type != "cuda":
        raise DudfError(f"generate_st: device must be a GPU (got {dev}); the HIP path has no CPU fallback")
    model = SIREN(n_in_features=3, n_out_features=1, hidden_layer_config=network_config["hidden_layer_nodes"],
                  w0=network_config["w0"], ww=network_config.get("ww"))
    model.load_state_dict(torch.load(network_config["model_path"], map_location=dev, weights_only=True))
    model.to(dev)
    return model, dev


def render(config_dict, jitter=None, colormap=None, model=None):
    """(height, width, 3) uint8: the image of reference generate_st.py:35-139 before PIL.  jitter: one value per pass (default: drawn
    from np.random.normal(0.5, 0.35) in the reference's call order); colormap: (256,3) table (default: matplotlib's RdYlBu, only
    fetched when curvatures are plotted); model: a loaded SIREN on the GPU instead of network_config['model_path']."""
    network_config, rendering_config = config_dict['network_config'], config_dict['rendering_config']
    passes = int(rendering_config['sample_rate'])
    if jitter is None:
        jitter = [np.random.normal(0.5, 0.35) for _ in range(passes)]
    jitter = [float(j) for j in np.atleast_1d(jitter)]
    if len(jitter) != passes or passes < 1:
        raise ValueError(f"sample_rate is {passes}; got {len(jitter)} jitter values")
    if network_config['gt_mode'] == 'gt':
        return _render_mesh(network_config, rendering_config, jitter)
    if model is None:
        model, dev = _load_model(network_config)
    else:
        dev = model.flat_parameters().device
        if dev.type != "cuda":
            raise DudfError(f"generate_st: the model must live on a GPU (got {dev}); the HIP path has no CPU fallback")
    height, width = int(rendering_config['height']), int(rendering_config['width'])
    lut = None
    if network_config['gt_mode'] != 'siren' and rendering_config.get('plot_curvatures', 'none') in ('mean', 'gaussian'):
        lut = np.ascontiguousarray(default_colormap() if colormap is None else colormap, dtype=np.float64)
        if lut.shape != (256, 3):
            raise DudfError(f"colormap must be a (256,3) array; got {lut.shape}")
        lut = torch.from_numpy(lut).to(dev)
    rotation = camera_rotation(rendering_config['camera_position'])
    cfg, theta = model.hip_cfg, model.flat_parameters()
    with torch.cuda.device(dev):
        acc = torch.zeros(height * width, 3, dtype=torch.float64, device=dev)
        for noise in jitter:
            hip_ops.render_pass(cfg, theta, noise, rotation, rendering_config['camera_position'], network_config, rendering_config,
                                lut, acc)
        image = hip_ops.render_finish(acc, passes)
    return image.cpu().numpy().reshape(height, width, 3)


def _device(network_config):
    dev = network_config.get("device", 0)
    dev = torch.device("cuda", dev) if isinstance(dev, int) else torch.device(dev)
    if dev.type != "cuda":
        raise DudfError(f"generate_st: device must be a GPU (got {dev}); the HIP path has no CPU fallback")
    return dev


def _mesh_path(path):
    """network_config['mesh_path'] as given, or — a relative path that is not there — relative to this script."""
    if os.path.isabs(path) or any(os.path.isfile(path + ext) for ext in ("", "_t.obj", ".obj")):
        return path
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), path)


def _render_mesh(network_config, rendering_config, jitter):
    """gt_mode 'gt' — reference generate_st.py:103-114 with the keys every other mode uses: the image of the mesh itself."""
    dev = _device(network_config)
    scene = load_scene(_mesh_path(network_config['mesh_path']), dev)
    height, width = int(rendering_config['height']), int(rendering_config['width'])
    rotation = camera_rotation(rendering_config['camera_position'])
    with torch.cuda.device(dev):
        acc = torch.zeros(height * width, 3, dtype=torch.float64, device=dev)
        for noise in jitter:
            rays, t0, mask = hip_ops.render_setup_rays(height, width, rendering_config['fov'], noise, rotation,
                                                       rendering_config['camera_position'],
                                                       rendering_config.get('planes', [1, -1, 1, -1, 1, -1]), dev)
            mesh_pass(scene, rays, t0, mask, rendering_config['light_position'], acc, bool(rendering_config.get('specular', False)),
                      rendering_config['surface_threshold'], rendering_config['max_iterations'])
        image = hip_ops.render_finish(acc, len(jitter))
    return image.cpu().numpy().reshape(height, width, 3)


def write_png(path, image):
    """8-bit RGB PNG of an (H,W,3) uint8 array with zlib alone (no PIL)."""
    image = np.ascontiguousarray(image, dtype=np.uint8)
    if image.ndim != 3 or image.shape[2] != 3:
        raise ValueError(f"write_png takes an (H,W,3) uint8 array; got {image.shape}")
    h, w = image.shape[:2]
    raw = np.concatenate([np.zeros((h, 1), np.uint8), image.reshape(h, w * 3)], axis=1).tobytes()     # filter type 0 per scanline

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def generate_st(config_dict):
    """reference generate_st.py:35-144: the PIL image (rotated by rendering_config['rotation']) — or, without PIL, the uint8 array."""
    image = render(config_dict)
    rotation = config_dict['rendering_config'].get('rotation', 0)
    try:
        from PIL import Image
    except ImportError:
        if rotation != 0:
            raise DudfError("rendering_config['rotation'] != 0 needs PIL (Image.rotate); it is not installed") from None
        return image
    im = Image.fromarray(image)
    if rotation != 0:
        im = im.rotate(rotation)
    return im


if __name__ == '__main__':
    parser = argparse.ArgumentParser(description='Generate ray traced image from trained model')
    parser.add_argument('config_path', metavar='path/to/json', type=str, help='path to render config')
    args = parser.parse_args()
    with open(args.config_path) as config_file:
        config_dict = json.load(config_file)
    im = generate_st(config_dict)
    out = config_dict["rendering_config"]["output_path"]
    if isinstance(im, np.ndarray):
        write_png(out, im)
    else:
        im.save(out, 'PNG')
    print(f'Saved to {out}')
