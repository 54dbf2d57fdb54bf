# coding: utf-8
"""GPU: normal orientation (diffudf_amd.metrics.orient_normals, csrc/dudf_orient.hip) against the numpy oracle of
tests/orient_oracle.py (pinned by tests/test_orient_cpu.py), fed with the DEVICE's k-NN indices: the minimum spanning forest under
the key (fp32 weight bits, slot) is unique, so flips, components and both counters must equal the oracle's exactly."""
import numpy as np
import pytest
import torch

import orient_oracle as OO
from diffudf_amd import hip_ops, metrics

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_knn(points, K):
    _, idx = metrics.knn_points(_cuda(points), _cuda(points), K, exclude_self=True)
    return idx


def check(points, normals, idx, what):
    """Runs the device twice on (points, normals, idx (device tensor)) and compares with the oracle; returns the device's result."""
    n = len(points)
    p, nr = _cuda(points), _cuda(normals)
    out, flip, comp, counts, stats = hip_ops.orient_normals(p, nr, idx)
    again = hip_ops.orient_normals(p, nr, idx)
    for a, b in zip((out, flip, comp, counts), again[:4]):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), what
    want = OO.orient(points, normals, idx.cpu().numpy())
    out, flip, comp, counts = out.cpu().numpy(), flip.cpu().numpy(), comp.cpu().numpy(), counts.tolist()
    print(f"{what}: n = {n}, {counts[0]} component(s), {counts[1]} forest edges, {stats['rounds']} rounds, {stats['launches']} launches")
    assert flip.dtype == np.uint8 and comp.dtype == np.int64 and out.dtype == np.float32
    assert counts == [want["components"], want["forest_edges"]] and counts[0] + counts[1] == n, what
    assert np.array_equal(comp, want["component"]), what
    assert np.array_equal(flip, want["flip"]), what
    assert np.array_equal(out.view(np.uint32), np.where(flip[:, None] == 1, -normals, normals).astype(np.float32).view(np.uint32)), what
    rounds_max = int(np.ceil(np.log2(max(n, 1)))) + 1
    assert 1 <= stats["rounds"] <= rounds_max, what
    return out, flip, comp, counts


def test_sphere():
    p, nrm = OO.sphere(4000)
    out, _, comp, counts = check(p, OO.random_flips(nrm), device_knn(p, 10), "sphere")
    assert counts[0] == 1 and (comp == 0).all()
    assert ((out * p).sum(axis=1) > 0).all()                      # oracle-free: every normal outward


def test_two_spheres():
    p, nrm = OO.two_spheres(3000)
    out, _, comp, counts = check(p, OO.random_flips(nrm), device_knn(p, 10), "two spheres")
    assert counts == [2, 5998] and set(np.unique(comp).tolist()) == {0, 3000}
    assert np.array_equal(out, nrm)


def test_torus():
    p, nrm = OO.torus(5000)
    out, _, comp, counts = check(p, OO.random_flips(nrm), device_knn(p, 10), "torus")
    assert counts[0] == 1 and OO.inconsistent(out, nrm, comp) == 0


def test_polyline_is_one_deep_chain():
    """K = 2: the graph is a path, the forest as deep as the cloud is long — what the pointer-doubling bound is for."""
    p, nrm = OO.polyline(5000)
    idx = device_knn(p, 2)
    out, _, comp, counts = check(p, OO.random_flips(nrm), idx, "polyline")
    assert counts == [1, 4999]
    assert ((out * nrm).sum(axis=1) > 0).all() or ((out * nrm).sum(axis=1) < 0).all()


def test_all_normals_equal():
    """Every weight is 0: the order of the edges is the slot number alone."""
    p, _ = OO.sphere(4000, seed=9)
    nrm = np.tile(np.array([[0.0, 0.6, -0.8]], dtype=np.float32), (len(p), 1))
    out, flip, _, counts = check(p, nrm, device_knn(p, 10), "equal normals")
    assert counts[0] == 1 and (flip == 1).all()                   # nobody disagrees; the seed's n_z < 0 flips the lot


def test_lattice_with_random_normals():
    p = OO.lattice(12, 1.0 / 8.0)
    g = np.random.default_rng(21).normal(size=p.shape)
    nrm = (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)
    check(p, nrm, device_knn(p, 6), "lattice, K = 6")
    check(p, nrm, device_knn(p, 16), "lattice, K = 16")


def test_padding_and_self_entries_are_no_edges():
    p, nrm = OO.sphere(4000, seed=5)
    idx = device_knn(p, 8).clone()
    rng = np.random.default_rng(23)
    mask = torch.from_numpy(rng.random((4000, 8)) < 0.3).to(DEV)
    idx[mask] = -1
    rows = torch.arange(4000, device=DEV)
    idx[rows[::3], 1] = rows[::3]                                  # self entries
    idx[7, 0] = 4000; idx[8, 2] = 1 << 40; idx[9, 3] = -(1 << 40)  # out of range either way: never dereferenced
    idx[100:140] = -1                                             # vertices with no slot of their own
    check(p, OO.random_flips(nrm), idx, "padded")
    tiny = np.zeros((3, 3), dtype=np.float32); tiny[:, 2] = (0.0, -0.0, 0.0)
    tn = np.array([[0, 0, -1], [0, 0, 1], [0, 0, 1]], dtype=np.float32)
    check(tiny, tn, torch.full((3, 2), -1, dtype=torch.int64, device=DEV), "no edges at all")


def test_one_point_and_none():
    p = np.array([[0.1, 0.2, 0.3]], dtype=np.float32)
    for nz in (-1.0, 1.0):
        nrm = np.array([[0.0, 0.0, nz]], dtype=np.float32)
        out, flip, comp, counts = check(p, nrm, device_knn(p, 10), "n = 1")
        assert out[0, 2] == 1.0 and counts == [1, 0] and comp.tolist() == [0]
    out = metrics.orient_normals(torch.zeros(0, 3, device=DEV), torch.zeros(0, 3, device=DEV))
    assert out.shape == (0, 3)


def test_in_place():
    p, nrm = OO.sphere(4000)
    fl = OO.random_flips(nrm)
    idx = device_knn(p, 10)
    buf = _cuda(fl)
    out, *_ = hip_ops.orient_normals(_cuda(p), buf, idx, out=buf)
    assert out.data_ptr() == buf.data_ptr() and np.array_equal(buf.cpu().numpy(), nrm)


def test_end_to_end_metrics_and_generate_pc():
    import generate_pc
    p, nrm = OO.sphere(4000)
    fl = OO.random_flips(nrm)
    out, info = metrics.orient_normals(_cuda(p), _cuda(fl), k=10, return_info=True)
    assert np.array_equal(out.cpu().numpy(), nrm)
    assert info["components"] == 1 and info["forest_edges"] == 3999 and int(info["flip"].sum()) == int((fl != nrm).any(axis=1).sum())
    pc = generate_pc.PointCloud(p, fl)
    assert pc.orient_normals_consistent_tangent_plane(10) is pc
    assert pc.normals.dtype == np.float32 and np.array_equal(pc.normals, nrm) and np.array_equal(pc.positions, p)
