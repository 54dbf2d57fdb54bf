# coding: utf-8
"""Reference src/preprocess_mesh.py without open3d: normalise a mesh or a point cloud and write the files training reads.

    preprocessMesh(outputPath, meshFile)          -> <name>_t.obj (normalised mesh)  + <name>_pc.ply (area-uniform surface cloud)
    preprocessPointCloud(outputPath, pcFile)      -> <name>_t.ply (normalised cloud) + <name>_pc.ply (subset without replacement)

Host numpy through `diffudf_amd.mesh`; only a raw scan needs the GPU (`preprocessPointCloud` estimates its normals and removes its
outliers there).  open3d's RNG stream is not reproduced, its distributions
are: the surface cloud comes from `mesh.sample_surface` (counter-based `synth.uniform01`), the subset from a counter-based
permutation; both are pure functions of (input, sample count, seed)."""
import os

import numpy as np

from . import mesh as dmesh
from . import synth
from ._lib import DudfError


class TriangleMesh:
    """`.vertices` (V,3) float64, `.triangles` (T,3) int64 — what the reference holds as an `o3d.geometry.TriangleMesh`."""

    def __init__(self, vertices, triangles):
        self.vertices = np.asarray(vertices, dtype=np.float64)
        self.triangles = np.asarray(triangles, dtype=np.int64)

    def get_center(self):
        return self.vertices.mean(axis=0)

    def transform(self, M):
        self.vertices = self.vertices @ M[:3, :3].T + M[:3, 3]


class PointCloud:
    """`.points`, `.normals` (P,3) float64 — the reference's `o3d.geometry.PointCloud`."""

    def __init__(self, points, normals):
        self.points = np.asarray(points, dtype=np.float64)
        self.normals = np.asarray(normals, dtype=np.float64)

    def get_center(self):
        return self.points.mean(axis=0)

    def transform(self, M):                       # a translation and a uniform scale: unit normals stay what they are
        self.points = self.points @ M[:3, :3].T + M[:3, 3]

    def normalize_normals(self):
        n = np.linalg.norm(self.normals, axis=1, keepdims=True)
        self.normals = self.normals / np.where(n > 0, n, 1.0)


def _normalize(obj, coords):
    """Centre on the mean, scale max|coord| to 1/1.1, in place; returns the 4x4 S @ T (reference :5-27)."""
    T = np.block([[np.eye(3, 3), -1 * obj.get_center().reshape((3, 1))], [np.eye(1, 4, k=3)]])
    obj.transform(T)
    max_coord = np.max(np.abs(coords(obj)))
    S = np.block([[np.eye(3, 3) * (1 / (max_coord + max_coord * 0.1)), np.zeros((3, 1))], [np.eye(1, 4, k=3)]])
    obj.transform(S)
    return S @ T


def normalizeMesh(mesh):
    return _normalize(mesh, lambda m: m.vertices)


def normalizePointCloud(pointCloud):
    return _normalize(pointCloud, lambda p: p.points)


def _name(path):
    return path[path.rfind('/') + 1: path.rfind('.')]


def preprocessMesh(outputPath, meshFile, surfacePoints=1e5, seed=123):
    """Writes <outputPath>/<name>_t.obj and <name>_pc.ply (reference :29-40); returns the normalising matrix."""
    vertices, triangles = dmesh.load_obj(meshFile)
    mesh = TriangleMesh(vertices, triangles)
    M = normalizeMesh(mesh)
    mesh_name = _name(meshFile)
    print(mesh_name)
    os.makedirs(outputPath, exist_ok=True)
    dmesh.write_obj(os.path.join(outputPath, mesh_name + '_t.obj'), mesh.vertices, mesh.triangles, fmt="%.17g")   # reads back exactly
    pos, nrm = dmesh.sample_surface(mesh.vertices, mesh.triangles, int(surfacePoints), seed)
    dmesh.write_ply_points(os.path.join(outputPath, mesh_name + '_pc.ply'), pos, nrm)
    return M


def preprocessPointCloud(outputPath, pcFile, surfacePoints=1e5, seed=123, estimate_normals=None, normals_k=15, remove_outliers=False,
                         nb_neighbors=16, std_ratio=2.0, device="cuda:0"):
    """Writes <outputPath>/<name>_t.ply (all points) and <name>_pc.ply (`surfacePoints` of them, no repeats; reference :42-66);
    returns the normalising matrix.

    A raw scan has no normals and may carry stray points; both steps run on `device` (diffudf_amd.metrics, imported only when asked
    for: a cloud with normals still needs no GPU).  remove_outliers: the statistical outlier test (nb_neighbors, std_ratio) on the
    cloud as read.  estimate_normals: None = when the file has none, True = always; normals_k neighbours, on the normalised cloud,
    oriented consistently.  Order: read, outlier removal, normalise, estimate and orient, subset, write."""
    pos, nrm = dmesh.read_ply_points(pcFile, require_normals=False)
    estimate = (nrm is None) if estimate_normals is None else bool(estimate_normals)
    if nrm is None and not estimate:
        raise DudfError(f"{pcFile} has no normals and estimate_normals=False: nothing to train on")
    removed = 0
    if remove_outliers:
        import torch
        from . import metrics
        _, kept, info = metrics.remove_statistical_outliers(torch.from_numpy(pos).to(device), nb_neighbors, std_ratio)
        kept, removed = kept.cpu().numpy(), info["removed"]
        pos, nrm = pos[kept], (None if nrm is None else nrm[kept])
    pointcloud = PointCloud(pos, np.zeros_like(pos) if estimate else nrm)
    if not estimate:
        pointcloud.normalize_normals()
    M = normalizePointCloud(pointcloud)
    pointcloud_name = _name(pcFile)
    print(pointcloud_name)
    components = None
    if estimate:                                  # on the float32 positions the files will hold
        import torch
        from . import metrics
        est, info = metrics.estimate_normals(torch.from_numpy(pointcloud.points.astype(np.float32)).to(device), k=normals_k, return_info=True)
        pointcloud.normals = est.cpu().numpy().astype(np.float64)
        components = info["orient"]["components"] if info["orient"] else 0
    if remove_outliers or estimate:
        print(f"{pointcloud_name}: {removed} outlier(s) removed, " +
              (f"normals estimated (k={int(normals_k)}), {components} orientation component(s)" if estimate else "normals kept from the file"))
    points, normals = pointcloud.points, pointcloud.normals
    if surfacePoints > len(points):
        raise ValueError(f'Cannot sample more points ({surfacePoints}) than present on the input pointcloud ({len(points)}).')
    # a permutation from one uniform per point (ties by index): its head is a sample without replacement
    indices = np.argsort(synth.uniform01(seed, 310, 0, len(points)), kind="stable")[:int(surfacePoints)]
    os.makedirs(outputPath, exist_ok=True)
    dmesh.write_ply_points(os.path.join(outputPath, pointcloud_name + '_t.ply'), points, normals)
    dmesh.write_ply_points(os.path.join(outputPath, pointcloud_name + '_pc.ply'), points[indices], normals[indices])
    return M
