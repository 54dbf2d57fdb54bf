#!/usr/bin/env python
# coding: utf-8
"""Quantitative evaluation — reference cuantitative.py: train one network per model of a dataset folder, extract the CAP-UDF and
MeshUDF meshes, and write L1 / L2 Chamfer distance and normal consistency of their vertices against the ground-truth cloud.

    python cuantitative.py [dataset] [outfolder] [device]        defaults: data/deepfashion/  results/df_subset/  0

The reference takes `chamfer_distance` from pytorch3d (a CUDA extension) and vertex normals and the cloud reader from open3d;
here the metric runs in `diffudf_amd.metrics` (HIP kernels: nearest neighbours on direct differences, the normal term, the
area-weighted vertex normals) and the cloud comes from `diffudf_amd.mesh.read_ply_points`.  The MeshUDF half needs the Lewiner
tables (generate_mc.py); without them its three columns are `nan`."""
import gc
import os
import sys

import numpy as np
import torch

from diffudf_amd import mesh as dmesh
from diffudf_amd import metrics as dmetrics

HEADER = 'mesh,time,L1CD_CAP,L2CD_CAP,NC_CAP,L1CD_MU,L2CD_MU,NC_MU'


class PointCloudFile:
    """`.points` / `.normals` of a `_pc.ply` cloud: what `o3d.io.read_point_cloud` hands the reference's `metrics`."""

    def __init__(self, path):
        self.points, self.normals = dmesh.read_ply_points(path)


class EvalMesh:
    """`mesh.as_open3d` + `compute_vertex_normals(normalized=True)` (reference :96-100): the vertices and faces of a trimesh /
    TriangleSoup mesh with AREA-weighted vertex normals computed on the device (trimesh's own `vertex_normals` weigh by angle)."""

    def __init__(self, mesh, cuda_device):
        self.vertices = np.asarray(mesh.vertices, dtype=np.float64)
        self.faces = np.asarray(mesh.faces, dtype=np.int64)
        self.vertex_normals = _area_normals(self.vertices, self.faces, _device(cuda_device)).cpu().numpy()


def _device(cuda_device):
    return torch.device("cuda", cuda_device) if isinstance(cuda_device, int) else torch.device(cuda_device)


def _area_normals(vertices, faces, dev):
    """(V,3) float32 on `dev`: `compute_vertex_normals(normalized=True)` (open3d, reference :99-100) of numpy vertices and faces."""
    return dmetrics.vertex_normals(torch.from_numpy(np.ascontiguousarray(vertices, dtype=np.float64)).to(dev),
                                   torch.from_numpy(np.ascontiguousarray(faces, dtype=np.int64)).to(dev))


def _vertex_normals(mesh, dev):
    n = getattr(mesh, "vertex_normals", None)
    if n is None:                                    # anything with .vertices and .faces: computed here
        return _area_normals(mesh.vertices, mesh.faces, dev)
    return torch.from_numpy(np.asarray(n)).float().to(dev)


def metrics(mesh, pointcloud, norm, cuda_device):
    """Reference cuantitative.py:10-19: (chamfer distance, normal consistency term) of the mesh's vertices against the cloud, as
    numpy scalars.  `mesh`: `.vertices` and `.vertex_normals` (or `.faces` to compute them from); `pointcloud`: `.points`,
    `.normals`."""
    dev = _device(cuda_device)
    t = lambda a: torch.from_numpy(np.asarray(a)).float()[None, ...].to(dev)   # noqa: E731
    cd, nc = dmetrics.chamfer_distance(x=t(mesh.vertices), y=t(pointcloud.points),
                                       x_normals=_vertex_normals(mesh, dev)[None, ...], y_normals=t(pointcloud.normals), norm=norm)
    return cd.cpu().numpy(), nc.cpu().numpy()


def default_exp_config(outfolder, net_width=256, net_depth=8):
    """The experiment of reference cuantitative.py:33-59."""
    return {
        "num_epochs": 3000,
        "s1_epochs": 2000,
        "warmup_epochs": 1000,
        "dataset": "...",
        "batch_size": 30000,
        "sampling_percentiles": [0.333, 0.666],
        "batches_per_epoch": 1,
        "checkpoint_path": outfolder,
        "experiment_name": "...",
        "epochs_to_checkpoint": 8001,
        "gt_mode": "tanh",
        "loss_s1_weights": [1e4, 1e4, 1e4, 1e3],
        "loss_s2_weights": [1e5, 1e5],
        "alpha": 10,
        "optimizer": {"type": "adam", "lr_s1": 1e-5, "lr_s2": 1e-7},
        "network": {"hidden_layer_nodes": [net_width] * net_depth, "w0": 30, "pretrained_dict": "None"},
        "resolution": 256,
    }


def run(dataset, outfolder, cuda_device, exp_config=None):
    """The loop of reference cuantitative.py:62-108: for every folder under `dataset` that holds a `*_pc.ply` and a `*_t.obj`, train
    (`setup_train`), then write one row of `results.csv` in `outfolder`.  Experiments whose folder exists are skipped.  Returns
    the rows written, as (name, time, L1CD_CAP, L2CD_CAP, NC_CAP, L1CD_MU, L2CD_MU, NC_MU, (mesh_MU, mesh_CAP)).  A training that
    returns no mesh raises RuntimeError naming the experiment (the reference fails there on its tuple unpacking)."""
    from train import setup_train
    if not os.path.exists(outfolder):
        os.mkdir(outfolder)
    exp_config = dict(default_exp_config(outfolder) if exp_config is None else exp_config)
    exp_config["checkpoint_path"] = outfolder
    csv = os.path.join(outfolder, 'results.csv')
    with open(csv, 'w+') as result_file:
        result_file.write(HEADER + '\n')
    rows = []
    for dirpath, dirnames, filenames in os.walk(dataset):
        clouds = [f for f in filenames if f.endswith('_pc.ply')]
        gts = [f for f in filenames if f.endswith('_t.obj')]
        if not clouds or not gts:
            continue
        # compared against the point cloud, not the vertices of the original mesh (reference :73)
        dataset_file = os.path.join(dirpath, clouds[0])
        print(f'Training for {gts[0]}')
        experiment_name = os.path.basename(os.path.normpath(dirpath))
        exp_config['dataset'] = dataset_file[:-7]
        exp_config['experiment_name'] = experiment_name
        if os.path.exists(os.path.join(outfolder, experiment_name)):
            print(f'Skipping {experiment_name}')
            continue
        training_time, meshes = setup_train(exp_config, cuda_device)
        if not meshes:
            raise RuntimeError(f"{experiment_name}: training produced no mesh (resolution 0, or no epoch improved on the initial loss)")
        if not isinstance(meshes, tuple):            # gt_mode 'siren' returns its one signed mesh: there is no MU / CAP pair to compare
            raise RuntimeError(f"{experiment_name}: the MU / CAP table needs gt_mode 'tanh' (got '{exp_config.get('gt_mode', 'tanh')}')")
        meshMU, meshCAP = meshes
        torch.cuda.empty_cache()
        gc.collect()

        print('Computing chamfer distances...')
        gt_pc = PointCloudFile(dataset_file)
        cap_mesh = EvalMesh(meshCAP, cuda_device)
        L1CD_CAP, NC_CAP = metrics(cap_mesh, gt_pc, norm=1, cuda_device=cuda_device)
        L2CD_CAP, _ = metrics(cap_mesh, gt_pc, norm=2, cuda_device=cuda_device)
        if meshMU is None:                           # no Lewiner tables: the CAP half still counts
            L1CD_MU = L2CD_MU = NC_MU = float('nan')
        else:
            mu_mesh = EvalMesh(meshMU, cuda_device)
            L1CD_MU, NC_MU = metrics(mu_mesh, gt_pc, norm=1, cuda_device=cuda_device)
            L2CD_MU, _ = metrics(mu_mesh, gt_pc, norm=2, cuda_device=cuda_device)
        with open(csv, 'a') as result_file:
            result_file.write(f'{experiment_name},{training_time},{L1CD_CAP},{L2CD_CAP},{NC_CAP},{L1CD_MU},{L2CD_MU},{NC_MU}\n')
        rows.append((experiment_name, training_time, L1CD_CAP, L2CD_CAP, NC_CAP, L1CD_MU, L2CD_MU, NC_MU, (meshMU, meshCAP)))
    return rows


if __name__ == '__main__':
    dataset = sys.argv[1] if len(sys.argv) > 1 else 'data/deepfashion/'
    outfolder = sys.argv[2] if len(sys.argv) > 2 else 'results/df_subset/'
    cuda_device = int(sys.argv[3]) if len(sys.argv) > 3 else 0
    run(dataset, outfolder, cuda_device)
