# coding: utf-8
"""GPU: `metrics.surface_metrics` on cases with a closed form, at n_samples = 4 096, and the `results_surface.csv` of
cuantitative.py.  Distances are fp32 results of fp32 coordinates below 2: a distance that is h in exact arithmetic comes back
within a few units of 2^-24 * max(h, |coordinate|), so 1e-6 absolute covers it."""
import os
import types

import numpy as np
import pytest
import torch

import surface_oracle as SO
from diffudf_amd import mesh, metrics, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
N = 4096
EPS = 1e-6


def _square(z, cells=1):
    """The unit square at height z as a cells x cells grid of right triangles: (vertices float64, faces int64)."""
    g = np.linspace(0.0, 1.0, cells + 1)
    X, Y = np.meshgrid(g, g, indexing="ij")
    v = np.stack([X.ravel(), Y.ravel(), np.full(X.size, z)], axis=1)
    i, j = np.meshgrid(np.arange(cells), np.arange(cells), indexing="ij")
    p = (i * (cells + 1) + j).ravel()
    f = np.stack([np.stack([p, p + cells + 1, p + cells + 2], axis=1), np.stack([p, p + cells + 2, p + 1], axis=1)], axis=1).reshape(-1, 3)
    return v, f.astype(np.int64)


def _icosphere(r, level):
    t = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, g = {}, []
        for a, b, c in f:
            m = []
            for p, q in ((a, b), (b, c), (c, a)):
                key = (min(p, q), max(p, q))
                if key not in mid:
                    w = v[p] + v[q]
                    mid[key] = len(v); v.append(w / np.linalg.norm(w))
                m.append(mid[key])
            g += [(a, m[0], m[2]), (b, m[1], m[0]), (c, m[2], m[1]), (m[0], m[1], m[2])]
        f = g
    return r * np.array(v), np.array(f, dtype=np.int64)


@pytest.fixture(scope="module")
def beetle():
    v, t = mesh.load_obj(os.path.join(HERE, "golden", "beetle.obj"))
    return mesh.normalize_vertices(v), t


def test_parallel_squares():
    h = 0.03
    rv, rf = _square(0.0)
    gv, gf = _square(h)
    cloud, cloud_n = metrics.sample_surface(gv, gf, N, seed=7)
    taus = (0.5 * h, h * (1.0 - 1e-4), h * (1.0 + 1e-4), 2.0 * h)
    m = metrics.surface_metrics(rv, rf, cloud, cloud_n, gt_mesh=(gv, gf), n_samples=N, taus=taus)
    for key in ("accuracy", "completeness", "chamfer_l1", "hausdorff"):
        assert abs(m[key] - h) <= EPS, key
    assert abs(m["chamfer_l2"] - h * h) <= 2.0 * h * EPS
    for k in ("precision", "recall", "fscore"):
        assert [m[k][t] for t in taus] == [0.0, 0.0, 1.0, 1.0], k
    assert abs(m["normal_consistency"] - 1.0) <= EPS
    assert m["n_samples"] == N and abs(m["area"] - 1.0) <= 1e-15
    # without the ground-truth mesh the accuracy direction measures to the nearest cloud point: at least h, and no normal is lost
    m2 = metrics.surface_metrics(rv, rf, cloud, cloud_n, n_samples=N, taus=taus)
    assert m2["accuracy"] >= h - EPS and m2["completeness"] == m["completeness"] and m2["recall"] == m["recall"]
    assert abs(m2["normal_consistency"] - 1.0) <= EPS
    # no normals on the ground-truth cloud: no normal consistency
    assert metrics.surface_metrics(rv, rf, cloud, None, n_samples=N, taus=taus)["normal_consistency"] is None
    # no cloud: the ground-truth mesh is sampled
    m3 = metrics.surface_metrics(rv, rf, None, gt_mesh=(gv, gf), n_samples=N, taus=taus)
    assert abs(m3["completeness"] - h) <= EPS and abs(m3["accuracy"] - h) <= EPS and abs(m3["normal_consistency"] - 1.0) <= EPS
    with pytest.raises(ValueError):
        metrics.surface_metrics(rv, rf, None, n_samples=N)


def test_mesh_against_samples_of_itself(beetle):
    v, f = beetle
    cloud, cloud_n = metrics.sample_surface(v, f, N, seed=31)
    m = metrics.surface_metrics(v, f, cloud, cloud_n, gt_mesh=(v, f), n_samples=N)
    assert 0.0 <= m["hausdorff"] <= EPS and 0.0 <= m["accuracy"] <= EPS and 0.0 <= m["completeness"] <= EPS
    assert m["chamfer_l2"] <= EPS * EPS
    assert list(m["fscore"].values()) == [1.0, 1.0] and list(m["fscore"]) == [0.005, 0.01]
    assert list(m["precision"].values()) == [1.0, 1.0] and list(m["recall"].values()) == [1.0, 1.0]
    assert abs(m["area"] - SO.area(v, f)) <= 1e-13 * m["area"]


def test_icosphere_against_a_larger_sphere():
    """A point at radius r + delta is at least delta from a mesh inscribed in the sphere of radius r, and at most delta + sagitta:
    its radial projection onto the mesh lies at a radius of r - sagitta or more.  The faces are acute triangles with corners on
    the sphere, so their circumradius is at most e / sqrt(3) for the longest edge e, and the sagitta r - sqrt(r^2 - e^2 / 3)."""
    r, delta = 0.5, 0.02
    v, f = _icosphere(r, 2)
    assert len(f) == 320
    e = max(np.linalg.norm(v[f[:, a]] - v[f[:, b]], axis=1).max() for a, b in ((0, 1), (1, 2), (2, 0)))
    sagitta = r - np.sqrt(r * r - e * e / 3.0)
    assert 0.0 < sagitta < 0.5 * delta
    d = np.stack([synth.normal01(3, k, 0, N) for k in range(3)], axis=1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    cloud = torch.from_numpy(((r + delta) * d).astype(np.float32)).to(DEV)
    normals = torch.from_numpy(d.astype(np.float32)).to(DEV)
    m = metrics.surface_metrics(v, f, cloud, normals, n_samples=N, taus=(delta - 1e-4, delta + sagitta + 1e-4))
    assert delta - EPS <= m["completeness"] <= delta + sagitta + EPS
    assert list(m["recall"].values()) == [0.0, 1.0]
    assert m["accuracy"] >= delta - EPS and m["hausdorff"] >= m["accuracy"]
    assert 0.0 <= m["normal_consistency"] <= 1.0 + EPS
    assert abs(m["area"] - SO.area(v, f)) <= 1e-13 * m["area"]
    # Normals, with the same icosphere at radius r + delta as the ground-truth mesh.  A face's points lie within alpha =
    # asin(rho / r) of its normal's direction (rho <= e / sqrt 3 its circumradius).  A query x and its closest point c on the other
    # mesh satisfy |x - c| <= (distance along the ray through x) and ||x| - |c|| >= that minus the other mesh's sagitta, so by the
    # law of cosines 2 |x| |c| (1 - cos theta) <= sagitta' (2 (delta + sagitta) - sagitta'): theta < 0.05 rad here.  The two normals
    # of a pair are therefore within 2 alpha + theta of each other (the cloud's radial normals within alpha + theta).
    R = r + delta
    sag2 = sagitta * R / r
    theta = np.arccos(1.0 - sag2 * (2.0 * (delta + sagitta) - sag2) / (2.0 * (r - sagitta) * (R - sag2)))
    alpha = np.arcsin(e / np.sqrt(3.0) / r)
    assert theta < 0.05 and alpha < 0.2
    m = metrics.surface_metrics(v, f, cloud, normals, gt_mesh=(v * (R / r), f), n_samples=N)
    assert np.cos(2.0 * alpha + theta) - EPS <= m["normal_consistency"] <= 1.0 + EPS     # 0.91; unrelated faces would give about 0.5


def test_missing_face_lowers_recall_only():
    """A 4 x 4 grid of the unit square (32 right triangles with legs a = 1/4) without one inner face, against a cloud of N samples
    of the whole grid.  A cloud point is farther than tau from the rest exactly when it lies in the hole's inner triangle at
    distance tau from its sides, which is the hole scaled by 1 - tau / rho about its incentre (rho = a (2 - sqrt 2) / 2 the
    inradius): a share p = (1 - tau / rho)^2 / 32 of the area.  The count of such points is binomial(N, p): 4 sigma."""
    gv, gf = _square(0.0, 4)
    hole = 13
    rf = np.delete(gf, hole, axis=0)
    cloud, cloud_n, face = metrics.sample_surface(gv, gf, N, seed=17, return_face=True)
    a = 0.25
    rho = a * (2.0 - np.sqrt(2.0)) / 2.0
    tau = 0.005
    assert tau < rho
    p = (1.0 - tau / rho) ** 2 / 32.0
    sigma = np.sqrt(p * (1.0 - p) / N)
    m = metrics.surface_metrics(gv, rf, cloud, cloud_n, gt_mesh=(gv, gf), n_samples=N, taus=(tau,))
    miss = 1.0 - m["recall"][tau]
    print(f"missing share {miss:.5f}, expected {p:.5f} +- {4 * sigma:.5f}; cloud points on the hole: {int((face == hole).sum())}")
    assert abs(miss - p) <= 4.0 * sigma
    assert 0.0 < miss <= float((face == hole).float().mean())            # only points of the hole can be missed
    assert m["precision"][tau] == 1.0 and m["accuracy"] <= EPS
    assert tau < m["hausdorff"] <= rho + EPS                             # the deepest point of the hole is its incentre
    full = metrics.surface_metrics(gv, gf, cloud, cloud_n, gt_mesh=(gv, gf), n_samples=N, taus=(tau,))
    assert full["recall"][tau] == 1.0 and full["fscore"][tau] == 1.0 and m["fscore"][tau] < 1.0
    assert abs(m["area"] - 31.0 / 32.0) <= 1e-14


def test_sample_to_sample_mode_is_chamfer_distance(beetle):
    """point_to_surface=False with a cloud only is the protocol of the other papers: both directions are nearest-neighbour
    distances between the samples and the cloud, which `chamfer_distance` (pinned by tests/test_chamfer_gpu.py) sums as squared
    distances.  Here each squared fp32 distance went through an fp32 square root and back (2 round-offs of 2^-24), and
    chamfer_distance returns fp32 (another one): 1e-6 relative."""
    v, f = beetle
    gv = v * 1.01 + 0.002
    cloud, cloud_n = metrics.sample_surface(gv, f, 5000, seed=99)
    m = metrics.surface_metrics(v, f, cloud, cloud_n, n_samples=N, seed=5, point_to_surface=False)
    samples, normals = metrics.sample_surface(v, f, N, seed=5)
    cd, cn = metrics.chamfer_distance(samples, cloud, x_normals=normals, y_normals=cloud_n, norm=2)
    assert abs(2.0 * m["chamfer_l2"] - float(cd)) <= 1e-6 * float(cd)
    assert abs(m["normal_consistency"] - (1.0 - 0.5 * float(cn))) <= 1e-6
    d_acc = torch.sqrt(metrics.nearest_points(samples, cloud)[0]); d_comp = torch.sqrt(metrics.nearest_points(cloud, samples)[0])
    assert abs(m["accuracy"] - float(d_acc.double().mean())) <= 1e-12 and abs(m["completeness"] - float(d_comp.double().mean())) <= 1e-12
    assert m["hausdorff"] == max(float(d_acc.max()), float(d_comp.max()))
    assert m["precision"][0.005] == float((d_acc.double() <= 0.005).double().mean()) and m["recall"][0.01] == float((d_comp.double() <= 0.01).double().mean())
    # and the default mode measures completeness to the surface itself: never more than to a sample of it
    assert metrics.surface_metrics(v, f, cloud, cloud_n, n_samples=N, seed=5)["completeness"] <= m["completeness"] + EPS


def test_cuantitative_surface_csv(tmp_path, monkeypatch):
    import cuantitative
    import train
    gv, gf = _square(0.0, 4)
    data = tmp_path / "data" / "sq"; os.makedirs(data)
    pos, nrm = mesh.sample_surface(gv, gf, 3000, seed=3)
    mesh.write_obj(str(data / "sq_t.obj"), gv, gf)
    mesh.write_ply_points(str(data / "sq_pc.ply"), pos, nrm)
    cap = types.SimpleNamespace(vertices=gv + np.array([0.0, 0.0, 0.004]), faces=gf)
    mu = types.SimpleNamespace(vertices=gv - np.array([0.0, 0.0, 0.008]), faces=np.delete(gf, 13, axis=0))
    taus = (0.005, 0.01)
    outs = {}
    for name, meshes, samples in (("plain", (mu, cap), 0), ("surface", (mu, cap), 512), ("no_mu", (None, cap), 512)):
        monkeypatch.setattr(train, "setup_train", lambda cfg, dev, meshes=meshes: (1.5, meshes))
        out = tmp_path / name
        rows = cuantitative.run(str(tmp_path / "data"), str(out), 0, exp_config=cuantitative.default_exp_config("x"),
                                surface_samples=samples, fscore_taus=taus)
        assert len(rows) == 1 and len(rows[0]) == 9 and rows[0][0] == "sq"
        outs[name] = out
    assert not os.path.exists(outs["plain"] / "results_surface.csv")
    assert open(outs["plain"] / "results.csv", "rb").read() == open(outs["surface"] / "results.csv", "rb").read()
    lines = open(outs["surface"] / "results_surface.csv").read().splitlines()
    assert lines[0] == cuantitative.surface_header(taus) and len(lines) == 2
    cells = lines[1].split(",")
    assert cells[0] == "sq" and len(cells) == len(lines[0].split(",")) == 25
    row = dict(zip(lines[0].split(","), cells))
    vals = {k: float(x) for k, x in row.items() if k != "mesh"}
    assert all(np.isfinite(x) for x in vals.values())
    assert abs(vals["accuracy_CAP"] - 0.004) <= EPS and abs(vals["completeness_CAP"] - 0.004) <= EPS and abs(vals["hausdorff_CAP"] - 0.004) <= EPS
    assert vals["precision@0.005_CAP"] == 1.0 and vals["fscore@0.005_CAP"] == 1.0 and abs(vals["NC_CAP"] - 1.0) <= EPS
    assert abs(vals["accuracy_MU"] - 0.008) <= EPS and vals["precision@0.005_MU"] == 0.0 and vals["fscore@0.005_MU"] == 0.0
    assert vals["precision@0.01_MU"] == 1.0 and 0.9 < vals["recall@0.01_MU"] < 1.0 and vals["completeness_MU"] > 0.008
    # the row is what surface_metrics returns for the CAP mesh
    pc = cuantitative.PointCloudFile(str(data / "sq_pc.ply"))
    want = metrics.surface_metrics(cap.vertices, cap.faces, pc.points, pc.normals, gt_mesh=(gv, gf), n_samples=512, taus=taus)
    assert cells[1:6] == [str(want[k]) for k in ("accuracy", "completeness", "chamfer_l1", "chamfer_l2", "hausdorff")]
    no_mu = open(outs["no_mu"] / "results_surface.csv").read().splitlines()[1].split(",")
    assert no_mu[1:13] == cells[1:13] and all(c == "nan" for c in no_mu[13:])
