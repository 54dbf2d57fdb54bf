#!/usr/bin/env python
# coding: utf-8
"""Dense oriented point cloud from a trained network — reference generate_pc.py:6-41.

    python generate_pc.py <config.json>     keys as the reference's: model_path, device, w0, hidden_layer_nodes, nsamples,
                                            ref_steps, surf_thresh, alpha, gt_mode, max_iter, output_path (+ optional "ww",
                                            "orient_normals": false writes the normals with the sign the eigensolver gave them)

With open3d installed the result is the reference's `o3d.t.geometry.PointCloud` (normals oriented with
`orient_normals_consistent_tangent_plane(10)`, written by `o3d.t.io.write_point_cloud`).  Without it `generate_pc` returns a
`PointCloud` of this module (positions + normals, float32) whose `orient_normals_consistent_tangent_plane(10)` runs on the device
(`diffudf_amd.metrics.orient_normals`: k-NN graph, minimum spanning forest, every connected component seeded at its highest
point), and the PLY is written here, binary little-endian."""
import argparse
import json

import numpy as np

from src.render_pc import Sampler
from diffudf_amd.mesh import write_ply_points


class PointCloud:
    """Stand-in for `o3d.t.geometry.PointCloud` when open3d is absent: float32 positions and normals, `write(path)`,
    `orient_normals_consistent_tangent_plane(k)`."""

    def __init__(self, positions, normals):
        self.positions = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        self.normals = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        if self.positions.shape != self.normals.shape:
            raise ValueError(f"positions {self.positions.shape} and normals {self.normals.shape} differ")

    def orient_normals_consistent_tangent_plane(self, k, device="cuda:0"):
        """Flip the normals in place so that neighbours agree (`diffudf_amd.metrics.orient_normals` with the k nearest neighbours of
        every point; each connected component of that graph ends with the normal of its highest point towards +z)."""
        import torch
        from diffudf_amd import metrics
        if len(self.positions) == 0:
            return self
        out = metrics.orient_normals(torch.from_numpy(self.positions).to(device), torch.from_numpy(self.normals).to(device), k=k)
        self.normals = np.ascontiguousarray(out.cpu().numpy(), dtype=np.float32)
        return self

    def write(self, path):
        write_ply_points(path, self.positions, self.normals)


def generate_pc(config):
    gen = Sampler(3, checkpoint=config['model_path'], device=config['device'], w0=config['w0'], ww=config.get('ww'),
                  hidden_layers=config["hidden_layer_nodes"])
    points, normals = gen.generate_point_cloud(
        num_points=config['nsamples'],
        num_steps=config['ref_steps'],
        surf_thresh=config['surf_thresh'],
        alpha=config['alpha'],
        gt_mode=config['gt_mode'],
        max_iter=config['max_iter']
    )
    try:
        import open3d as o3d
    except ImportError:
        return PointCloud(points, normals)
    device = o3d.core.Device("CUDA:" + str(config['device'])) if isinstance(config['device'], int) else o3d.core.Device("CPU:0")
    dtype = o3d.core.float32
    pcd = o3d.t.geometry.PointCloud(device)
    pcd.point.positions = o3d.core.Tensor(points, dtype, device)
    pcd.point.normals = o3d.core.Tensor(normals, dtype, device)
    return pcd


if __name__ == '__main__':
    parser = argparse.ArgumentParser(description='Generate dense point cloud from trained model')
    parser.add_argument('config_path', metavar='path/to/json', type=str, help='path to render config')
    args = parser.parse_args()
    with open(args.config_path) as config_file:
        config_dict = json.load(config_file)
    point_cloud = generate_pc(config_dict)
    if isinstance(point_cloud, PointCloud):
        if config_dict.get("orient_normals", True):
            dev = config_dict['device']
            point_cloud.orient_normals_consistent_tangent_plane(10, device=f"cuda:{dev}" if isinstance(dev, int) else "cuda:0")
        point_cloud.write(config_dict['output_path'])
    else:
        import open3d as o3d
        point_cloud.orient_normals_consistent_tangent_plane(10)
        o3d.t.io.write_point_cloud(config_dict['output_path'], point_cloud)
