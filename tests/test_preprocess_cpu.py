# coding: utf-8
"""CPU: preprocess.py / src.preprocess_mesh — the files training and cuantitative.py read, written without open3d."""
import os
import shutil

import numpy as np
import pytest

import preprocess
from cuantitative import PointCloudFile
from diffudf_amd import mesh
from oracle.sampler_oracle import point_triangle_dist2
from src.preprocess_mesh import TriangleMesh, normalizeMesh, preprocessMesh, preprocessPointCloud

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BEETLE = os.path.join(GOLDEN, "beetle.obj")
N = 2000


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    out = tmp_path_factory.mktemp("pre")
    preprocess.main([BEETLE, str(out), "-s", str(N)])
    return str(out)


def test_mesh_is_centred_and_scaled(pair):
    v, t = mesh.load_obj(os.path.join(pair, "beetle_t.obj"))
    v0, t0 = mesh.load_obj(BEETLE)
    assert np.array_equal(t, t0)
    assert np.abs(v.mean(axis=0)).max() <= 1e-12
    assert np.abs(v).max() == pytest.approx(1 / 1.1, rel=1e-12)


def test_returned_matrix_maps_input_to_output(pair, tmp_path):
    M = preprocessMesh(str(tmp_path), BEETLE, surfacePoints=10)
    v0, _ = mesh.load_obj(BEETLE)
    v, _ = mesh.load_obj(os.path.join(str(tmp_path), "beetle_t.obj"))
    mapped = (M @ np.concatenate([v0, np.ones((len(v0), 1))], axis=1).T).T
    assert np.allclose(mapped[:, 3], 1.0)
    assert np.abs(mapped[:, :3] - v).max() <= 1e-12
    m = TriangleMesh(*mesh.load_obj(BEETLE))                     # the in-memory form returns the same matrix
    assert np.array_equal(normalizeMesh(m), M) and np.array_equal(m.vertices, v)


def test_cloud_lies_on_the_mesh_with_triangle_normals(pair):
    v, t = mesh.load_obj(os.path.join(pair, "beetle_t.obj"))
    tri64 = np.concatenate([v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]], axis=1)
    pos, nrm = mesh.read_ply_points(os.path.join(pair, "beetle_pc.ply"))
    assert pos.shape == (N, 3) and nrm.shape == (N, 3) and pos.dtype == np.float32
    d2 = np.concatenate([point_triangle_dist2(pos[i:i + 500].astype(np.float64), tri64) for i in range(0, N, 500)])
    d = np.sqrt(d2.min(axis=1))
    bound = 4 * np.finfo(np.float32).eps * np.abs(v).max()       # points are stored as fp32
    assert d.max() <= bound, (d.max(), bound)
    assert np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1).max() <= 4 * np.finfo(np.float32).eps
    n_tri, _ = mesh.triangle_normals_areas(v, t)
    attains = d2 <= (d[:, None] + bound) ** 2                    # triangles within the storage error of the minimum
    err = np.abs(nrm[:, None, :].astype(np.float64) - n_tri[None]).max(axis=2)
    best = np.where(attains, err, np.inf).min(axis=1)
    assert best.max() <= 2 * np.finfo(np.float32).eps, best.max()


def test_same_seed_same_files_other_seed_other_cloud(pair, tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    preprocess.main([BEETLE, a, "-s", str(N)])
    preprocess.main([BEETLE, b, "-s", str(N), "--seed", "7"])
    for name in ("beetle_t.obj", "beetle_pc.ply"):
        assert open(os.path.join(a, name), "rb").read() == open(os.path.join(pair, name), "rb").read()
    assert open(os.path.join(a, "beetle_t.obj"), "rb").read() == open(os.path.join(b, "beetle_t.obj"), "rb").read()
    pa, _ = mesh.read_ply_points(os.path.join(a, "beetle_pc.ply"))
    pb, _ = mesh.read_ply_points(os.path.join(b, "beetle_pc.ply"))
    assert not np.array_equal(pa, pb)


def test_pair_reads_back(pair):
    pc = PointCloudFile(os.path.join(pair, "beetle_pc.ply"))
    assert pc.points.shape == (N, 3) and pc.normals.shape == (N, 3)
    tri, pos, nrm = mesh.prepare(os.path.join(pair, "beetle"))
    v, t = mesh.load_obj(os.path.join(pair, "beetle_t.obj"))
    assert np.array_equal(tri, mesh.triangle_soup(v, t))          # read, not normalised a second time
    assert np.array_equal(pos, pc.points) and np.array_equal(nrm, pc.normals)
    none, pos2, _ = mesh.prepare(os.path.join(pair, "beetle"), cloud_only=True)
    assert none is None and np.array_equal(pos2, pos)


def test_point_cloud_subset(pair, tmp_path):
    src = os.path.join(str(tmp_path), "cloud.ply")
    pos, nrm = mesh.read_ply_points(os.path.join(pair, "beetle_pc.ply"))
    mesh.write_ply_points(src, pos * 3.0 + 1.0, nrm * 2.0)        # off-centre, normals not unit
    out = str(tmp_path / "out")
    M = preprocessPointCloud(out, src, surfacePoints=500)
    full, fn = mesh.read_ply_points(os.path.join(out, "cloud_t.ply"))
    sub, sn = mesh.read_ply_points(os.path.join(out, "cloud_pc.ply"))
    assert full.shape == (N, 3) and sub.shape == (500, 3)
    assert np.abs(full.astype(np.float64).mean(axis=0)).max() <= 1e-6 and np.abs(full).max() == pytest.approx(1 / 1.1, rel=1e-6)
    assert np.abs(np.linalg.norm(fn.astype(np.float64), axis=1) - 1).max() <= 4 * np.finfo(np.float32).eps
    src_pos = mesh.read_ply_points(src)[0].astype(np.float64)
    mapped = src_pos @ M[:3, :3].T + M[:3, 3]
    assert np.abs(mapped - full).max() <= 4 * np.finfo(np.float32).eps
    rows = {r.tobytes(): i for i, r in enumerate(np.concatenate([full, fn], axis=1))}
    assert len(rows) == N                                         # the input rows are distinct, so a row identifies its point
    picked = [rows[r.tobytes()] for r in np.concatenate([sub, sn], axis=1)]     # KeyError: not a row of the input (or its normal strayed)
    assert len(set(picked)) == 500
    out2 = str(tmp_path / "out2")
    preprocessPointCloud(out2, src, surfacePoints=500)
    assert open(os.path.join(out2, "cloud_pc.ply"), "rb").read() == open(os.path.join(out, "cloud_pc.ply"), "rb").read()
    preprocessPointCloud(out2, src, surfacePoints=500, seed=7)
    assert not np.array_equal(mesh.read_ply_points(os.path.join(out2, "cloud_pc.ply"))[0], sub)
    with pytest.raises(ValueError, match=r"Cannot sample more points \(2001\) than present on the input pointcloud \(2000\)\."):
        preprocessPointCloud(out2, src, surfacePoints=N + 1)
    preprocess.main([src, str(tmp_path / "cli"), "-pc", "-s", "100"])
    assert mesh.read_ply_points(str(tmp_path / "cli" / "cloud_pc.ply"))[0].shape == (100, 3)


def test_directory_walk_skips_outputs(pair, tmp_path):
    root = tmp_path / "data"
    (root / "a").mkdir(parents=True)
    shutil.copy(BEETLE, str(root / "a" / "bug.obj"))
    shutil.copy(os.path.join(pair, "beetle_t.obj"), str(root / "a" / "old_t.obj"))
    shutil.copy(BEETLE, str(root / "a" / "old_pc.obj"))
    preprocess.main([str(root), "unused", "-s", "50"])
    made = sorted(os.path.relpath(os.path.join(d, f), str(root)) for d, _, fs in os.walk(str(root)) for f in fs)
    assert made == ["a/bug.obj", "a/bug/bug_pc.ply", "a/bug/bug_t.obj", "a/old_pc.obj", "a/old_t.obj"]
    shutil.copy(os.path.join(pair, "beetle_pc.ply"), str(root / "a" / "scan.ply"))
    shutil.copy(os.path.join(pair, "beetle_pc.ply"), str(root / "a" / "scan_t.ply"))     # an output of an earlier run
    preprocess.main([str(root), "unused", "-pc", "-s", "50"])
    assert mesh.read_ply_points(str(root / "a" / "scan_pc.ply"))[0].shape == (50, 3)
    assert not os.path.exists(str(root / "a" / "scan_t_pc.ply")) and not os.path.exists(str(root / "a" / "bug" / "bug_pc_pc.ply"))
