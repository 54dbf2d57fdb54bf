#!/usr/bin/env python
# coding: utf-8
"""Field slice of a trained network — the query half of reference generate_df.py:50-148 (`generate_df`):

    python generate_df.py path/to/mesh.obj path/to/model.pth path/to/output/ [-d 0] [-w0 30] [-w 512] [-t 1e-3]
                          [--gt_mode siren] [-a 1] [-pc]                 (the reference's CLI, generate_df.py:248-266)

`field_slice(model, options)` samples the reference's plane (:68-79: `width`^2 points, first coordinate fixed at 0, the other
two running from +1 to -1), evaluates value, gradient and Hessian with the HIP query kernels (`src.evaluate.evaluate`,
one call), and derives what the reference draws: the predicted value, |grad f| and the normal map — normalised gradient,
replaced by the sign-aligned top Hessian eigenvector where the RAW gradient is shorter than 0.04 (:84-100; note the
raw norm, unlike `extract_fields`), third component made non-negative, mapped to RGB (:105-107).

This is the parity artefact of SURVEY.md §8(f) ("learned field samples and grad f on a fixed grid"): the three arrays
are checked against the reference's own outputs in tests/golden/g9_slice.npz.  The ground-truth panels of the figure
(:108-127) take the distance of every slice point to the mesh — open3d's RaycastingScene in the reference,
`diffudf_amd.metrics.MeshIndex` (a bounding-volume hierarchy on the device) here; `generate_df_pc` (:150-245) takes the
distance to the nearest point of a cloud instead (`-pc`).  Without a mesh the figure holds the two predicted panels.
"""
import argparse

import numpy as np
import torch

from src.evaluate import evaluate
from src.model import SIREN
from src.util import normalize


def slice_samples(width, bordes=(1, -1), ejeplano=(2, 1, 0), offsetplano=0.0):
    """(width^2, 3) sample plane exactly as reference generate_df.py:68-79 builds it."""
    ranges = np.linspace(bordes[0], bordes[1], width)
    i_1, i_2 = np.meshgrid(ranges, ranges)
    planes = np.array([np.expand_dims(i_1, 2), np.expand_dims(i_2, 2), np.expand_dims(np.ones_like(i_1) * offsetplano, 2)])
    return np.concatenate(np.concatenate(planes[list(ejeplano)], axis=2), axis=0)


def field_slice(model, options):
    """dict(samples, pred_distances (S,1), pred_grad_norm (S,1), normals (S,3), grad_map (W,W,3) uint8)."""
    width = options['width']
    samples = slice_samples(width)
    n = width * width
    gradients = np.zeros((n, 3)); hessians = np.zeros((n, 3, 3))
    dev = torch.device(options.get('device', 'cuda:0'))
    pred = evaluate(model, samples, device=dev, gradients=gradients, hessians=hessians)
    gnorm = np.linalg.norm(gradients, axis=1).reshape((n, 1))
    g = normalize(gradients)
    # top eigenvector of the Hessian's lower triangle, as torch.linalg.eigh reads it (reference :86-87)
    lam, V = np.linalg.eigh(hessians, UPLO='L')
    pn = V[..., 2]
    pn = np.where(np.sum(g * pn, axis=-1)[..., None] < 0, -1.0, 1.0) * pn
    normals = np.where(np.concatenate([gnorm, gnorm, gnorm], axis=-1) < 0.04, pn, g)
    normals = normals * np.hstack([np.ones((n, 2)), np.sign(normals[:, 2]).reshape((n, 1))])
    grad_map = (((normals + np.ones_like(normals)) / 2).reshape(width, width, 3) * 255).astype(np.uint8)
    return {"samples": samples, "pred_distances": pred, "pred_grad_norm": gnorm, "normals": normals, "grad_map": grad_map}


def ground_truth(distances, options):
    """(value, gradient norm) of the ground-truth function of `gt_mode` at unsigned distances d (reference :111-122)."""
    d = np.asarray(distances).reshape(-1, 1)
    if options['gt_mode'] == 'squared':
        return options['alpha'] * (d ** 2), 2 * options['alpha'] * d
    if options['gt_mode'] == 'tanh':
        t = np.tanh(options['alpha'] * d)
        return d * t, t + options['alpha'] * d * (1 - t ** 2)
    if options['gt_mode'] == 'siren':
        return d, np.where(d < options['surf_thresh'], np.zeros_like(d), np.ones_like(d))
    raise ValueError('gt_mode not valid')


def mesh_distances(mesh_path, samples, device):
    """Distance of the samples, as fp32 (reference :110), to the triangles of an OBJ: `diffudf_amd.metrics.MeshIndex` in place of
    open3d's RaycastingScene (:108-110).  (S,1) float32."""
    from diffudf_amd import mesh as dmesh, metrics
    vertices, triangles = dmesh.load_obj(mesh_path)
    scene = metrics.MeshIndex(vertices, triangles, device=device)
    pts = torch.from_numpy(np.ascontiguousarray(samples, dtype=np.float32)).to(device)
    return scene.distance(pts).cpu().numpy().reshape(-1, 1)


def cloud_distances(pc_path, samples, device):
    """Distance of the samples, as fp32, to the nearest point of a PLY cloud: `metrics.nearest_points` in place of the KD-tree of
    reference :205-206.  (S,1) float32."""
    from diffudf_amd import mesh as dmesh, metrics
    pos, _ = dmesh.read_ply_points(pc_path, require_normals=False)
    pts = torch.from_numpy(np.ascontiguousarray(samples, dtype=np.float32)).to(device)
    d2, _ = metrics.nearest_points(pts, torch.from_numpy(pos).to(device), norm=2)
    return torch.sqrt(d2.double()).float().cpu().numpy().reshape(-1, 1)


def _load_model(model_path, options):
    model = SIREN(n_in_features=3, n_out_features=1, hidden_layer_config=options['hidden_layer_nodes'],
                  w0=options['weight0'], ww=None, activation=options.get('activation', 'sine'))
    model.load_state_dict(torch.load(model_path, weights_only=True))
    model.to(torch.device(options.get('device', 'cuda:0')))
    return model


def _with_ground_truth(out, distances, options):
    """The ground-truth side of the slice: `gt_distances` (the unsigned distance itself), `gt_values` / `gt_grad_norm` (the function
    of `gt_mode` the network was trained towards and the norm of its gradient: what the upper panels show) and `field_l1`, the mean
    |pred - gt_values| over the slice."""
    out["gt_distances"] = distances
    out["gt_values"], out["gt_grad_norm"] = ground_truth(distances, options)
    out["field_l1"] = np.float64(np.mean(np.abs(out["pred_distances"].reshape(-1) - out["gt_values"].reshape(-1).astype(np.float64))))
    return out


def _write(out, output_path, options, gt_distances=None):
    np.savez_compressed(output_path + 'field_slice.npz', **out)
    from PIL import Image
    Image.fromarray(out["grad_map"]).save(output_path + 'pred_grad.png', 'PNG')
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:                                   # pragma: no cover
        return out
    w = options['width']
    panels = [("Predicted value slice", np.clip(out["pred_distances"], None, 1.5)),
              (r"$\|\nabla f\|$", np.clip(out["pred_grad_norm"], None, 1.5))]
    if "gt_values" in out:                                # the reference's four panels (:132-138): truth left, prediction right
        panels = [("Ground truth slice", np.clip(out["gt_values"], None, 1.5)), panels[0],
                  ("Ground truth gradient norm", np.clip(out["gt_grad_norm"], None, 1.5)), panels[1]]
    elif gt_distances is not None:
        d = np.asarray(gt_distances).reshape(-1, 1)
        if options['gt_mode'] == 'tanh':
            t = np.tanh(options['alpha'] * d)
            panels = [("Ground truth slice", np.clip(d * t, None, 1.5)),
                      ("Ground truth gradient norm", np.clip(t + options['alpha'] * d * (1 - t ** 2), None, 1.5))] + panels
    fig, axes = plt.subplots(nrows=len(panels) // 2, ncols=2, figsize=(10, 4.5 * (len(panels) // 2)), dpi=200, squeeze=False)
    for ax, (title, img) in zip(axes.flat, panels):
        pos = ax.imshow(img.reshape(w, w), cmap='bwr_r', interpolation='none', vmin=-1.5, vmax=1.5)
        ax.contour(np.ma.masked_outside(img, -options.get('surf_thresh', 0.01), options.get('surf_thresh', 0.01)).reshape(w, w),
                   colors='black', linewidths=0.5)
        ax.set_title(title); ax.set_xticks([]); ax.set_yticks([])
    fig.colorbar(pos, ax=axes.ravel().tolist(), shrink=0.8)
    fig.savefig(output_path + 'distance_fields.png')
    plt.close(fig)
    return out


def generate_df(model_path, mesh_path, output_path, options, gt_distances=None):
    """Reference signature (generate_df.py:50).  With `mesh_path` a readable .obj (and no `gt_distances`) the ground truth of the
    slice is computed on the device (`mesh_distances`): the figure gets the reference's four panels and field_slice.npz the keys of
    `_with_ground_truth`.  `mesh_path=None`: the two predicted panels only; explicit `gt_distances`: the caller's distances in the
    upper panels ('tanh' only), nothing added to the file."""
    import os
    out = field_slice(_load_model(model_path, options), options)
    if gt_distances is None and mesh_path is not None and str(mesh_path).lower().endswith('.obj') and os.path.isfile(mesh_path):
        _with_ground_truth(out, mesh_distances(mesh_path, out["samples"], options.get('device', 'cuda:0')), options)
    return _write(out, output_path, options, gt_distances)


def generate_df_pc(model_path, pc_path, output_path, options):
    """Reference generate_df.py:150-245: the same slice with the distance to the nearest point of the cloud `pc_path` (a PLY) as
    ground truth."""
    out = field_slice(_load_model(model_path, options), options)
    _with_ground_truth(out, cloud_distances(pc_path, out["samples"], options.get('device', 'cuda:0')), options)
    return _write(out, output_path, options)


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description='Field slice of a trained model')
    parser.add_argument('mesh_path', metavar='path/to/mesh.obj', type=str,
                        help='path to input preprocessed mesh <name>_t.obj (ground-truth panels); with -pc the cloud <name>_t.ply')
    parser.add_argument('model_path', metavar='path/to/pth', type=str, help='path to input model')
    parser.add_argument('output_path', metavar='path/to/output/', type=str, help='path to output folder')
    parser.add_argument('-d', '--device', type=int, default=0, help='torch device')
    parser.add_argument('-w0', '--weight0', type=float, default=30, help='w0 parameter of SIREN')
    parser.add_argument('-w', '--width', type=int, default=512, help='width of generated image')
    parser.add_argument('-t', '--surf_thresh', type=float, default=1e-3, help='on surface threshold')
    parser.add_argument('--gt_mode', type=str, default='siren', help='ground truth function')
    parser.add_argument('-a', '--alpha', type=float, default=1, help='alpha for ground truth')
    parser.add_argument('-pc', '--pointcloud', action='store_true', help='the ground truth is a point cloud (PLY): generate_df_pc')
    args = parser.parse_args()
    d = vars(args)
    d['hidden_layer_nodes'] = [256] * 8
    d['activation'] = 'sine'
    d['device'] = f"cuda:{args.device}"
    (generate_df_pc if args.pointcloud else generate_df)(args.model_path, args.mesh_path, args.output_path, d)
