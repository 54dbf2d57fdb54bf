#!/usr/bin/env python
# coding: utf-8
"""Quantitative evaluation — reference cuantitative.py: train one network per model of a dataset folder, extract the CAP-UDF and
MeshUDF meshes, and write L1 / L2 Chamfer distance and normal consistency of their vertices against the ground-truth cloud.

    python cuantitative.py [dataset] [outfolder] [device]        defaults: data/deepfashion/  results/df_subset/  0
    python cuantitative.py data/deepfashion/ results/df_subset/ 0 --surface-samples 100000 --fscore-taus 0.005,0.01

The reference takes `chamfer_distance` from pytorch3d (a CUDA extension) and vertex normals and the cloud reader from open3d;
here the metric runs in `diffudf_amd.metrics` (HIP kernels: nearest neighbours on direct differences, the normal term, the
area-weighted vertex normals) and the cloud comes from `diffudf_amd.mesh.read_ply_points`.  The MeshUDF half needs the Lewiner
tables (generate_mc.py); without them its three columns are `nan`.

`--surface-samples N` (off by default) adds the protocol of CAP-UDF, MeshUDF and NDF in a second file, `results_surface.csv`: N
area-uniform samples of each extracted surface against the ground truth — accuracy, completeness, L1 / L2 Chamfer distance,
Hausdorff distance, precision / recall / F-score at the thresholds of `--fscore-taus`, normal consistency
(`diffudf_amd.metrics.surface_metrics`).  `results.csv` is the same file with and without it."""
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


def surface_header(taus):
    """The header of `results_surface.csv` for the thresholds `taus`."""
    cols = ['mesh']
    for half in ('CAP', 'MU'):
        cols += [f'{k}_{half}' for k in ('accuracy', 'completeness', 'chamfer_l1', 'chamfer_l2', 'hausdorff')]
        cols += [f'{k}@{t}_{half}' for k in ('precision', 'recall', 'fscore') for t in taus]
        cols.append(f'NC_{half}')
    return ','.join(cols)


def surface_fields(mesh, gt_pc, gt_mesh, surface_samples, taus, cuda_device):
    """The values of one half (CAP or MU) of a `results_surface.csv` row, in header order; all NaN for `mesh` None."""
    if mesh is None:
        return [float('nan')] * (6 + 3 * len(taus))
    dev = _device(cuda_device)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)   # noqa: E731
    m = dmetrics.surface_metrics(up(np.asarray(mesh.vertices), torch.float64), up(np.asarray(mesh.faces), torch.int64),
                                 up(gt_pc.points, torch.float32), up(gt_pc.normals, torch.float32),
                                 gt_mesh=None if gt_mesh is None else (up(gt_mesh[0], torch.float64), up(gt_mesh[1], torch.int64)),
                                 n_samples=surface_samples, taus=taus)
    nc = m['normal_consistency']
    return ([m[k] for k in ('accuracy', 'completeness', 'chamfer_l1', 'chamfer_l2', 'hausdorff')]
            + [m[k][t] for k in ('precision', 'recall', 'fscore') for t in taus] + [float('nan') if nc is None else nc])


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


def run(dataset, outfolder, cuda_device, exp_config=None, surface_samples=0, fscore_taus=(0.005, 0.01)):
    """The loop of reference cuantitative.py:62-108: for every folder under `dataset` that holds a `*_pc.ply` and a `*_t.obj`, train
    (`setup_train`), then write one row of `results.csv` in `outfolder`.  Experiments whose folder exists are skipped.  Returns
    the rows written, as (name, time, L1CD_CAP, L2CD_CAP, NC_CAP, L1CD_MU, L2CD_MU, NC_MU, (mesh_MU, mesh_CAP)).  A training that
    returns no mesh raises RuntimeError naming the experiment (the reference fails there on its tuple unpacking).
    surface_samples > 0: every experiment also appends a row to `results_surface.csv` (`surface_header(fscore_taus)`): the
    surface-sampled metrics of the CAP and MU meshes against the `_pc.ply` cloud and, for the accuracy direction, the `_t.obj` mesh
    beside it.  `results.csv` and the returned rows do not change.  `exp_config` goes to `setup_train` as it is, this repository's
    own keys included (`"hip_graph"`, `"sampler_index"`: train.py)."""
    from train import setup_train
    if not os.path.exists(outfolder):
        os.mkdir(outfolder)
    exp_config = dict(default_exp_config(outfolder) if exp_config is None else exp_config)
    exp_config["checkpoint_path"] = outfolder
    csv = os.path.join(outfolder, 'results.csv')
    with open(csv, 'w+') as result_file:
        result_file.write(HEADER + '\n')
    fscore_taus = tuple(float(t) for t in fscore_taus)
    surface_csv = os.path.join(outfolder, 'results_surface.csv')
    if surface_samples > 0:
        with open(surface_csv, 'w+') as result_file:
            result_file.write(surface_header(fscore_taus) + '\n')
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
        if surface_samples > 0:
            print('Computing surface-sampled metrics...')
            gt_mesh = dmesh.load_obj(os.path.join(dirpath, gts[0]))
            fields = [v for mesh in (meshCAP, meshMU)
                      for v in surface_fields(mesh, gt_pc, gt_mesh, surface_samples, fscore_taus, cuda_device)]
            with open(surface_csv, 'a') as result_file:
                result_file.write(','.join([experiment_name] + [str(v) for v in fields]) + '\n')
        rows.append((experiment_name, training_time, L1CD_CAP, L2CD_CAP, NC_CAP, L1CD_MU, L2CD_MU, NC_MU, (meshMU, meshCAP)))
    return rows


def parse_args(argv):
    """(dataset, outfolder, cuda_device, surface_samples, fscore_taus) of a command line: up to three positionals as the reference
    takes them, then `--surface-samples N` and `--fscore-taus a,b`."""
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('dataset', nargs='?', default='data/deepfashion/')
    ap.add_argument('outfolder', nargs='?', default='results/df_subset/')
    ap.add_argument('device', nargs='?', type=int, default=0)
    ap.add_argument('--surface-samples', type=int, default=0, metavar='N')
    ap.add_argument('--fscore-taus', default='0.005,0.01', metavar='a,b')
    a = ap.parse_args(argv)
    return a.dataset, a.outfolder, a.device, a.surface_samples, tuple(float(t) for t in a.fscore_taus.split(',') if t)


if __name__ == '__main__':
    dataset, outfolder, cuda_device, surface_samples, fscore_taus = parse_args(sys.argv[1:])
    run(dataset, outfolder, cuda_device, surface_samples=surface_samples, fscore_taus=fscore_taus)
