# coding: utf-8
"""CPU: the float64 oracle of the Chamfer tests is pinned (scipy's cKDTree, a hand-computed case), and everything of the new
surface that needs no device: workspace sizes, argument errors of the C entry points, `cuantitative` importable without
pytorch3d / open3d, no CPU fallback, no silently ignored keyword."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chamfer_oracle as CO  # noqa: E402

from diffudf_amd import _lib  # noqa: E402

NULL = ctypes.c_void_p(0)


@pytest.mark.parametrize("norm", [1, 2])
def test_oracle_agrees_with_ckdtree(norm):
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(7)
    x = rng.uniform(-0.9, 0.9, (3000, 3)).astype(np.float32)
    y = rng.uniform(-0.9, 0.9, (2500, 3)).astype(np.float32)
    d1, i1, d2 = CO.nearest(x, y, norm)
    dk, ik = cKDTree(y.astype(np.float64)).query(x.astype(np.float64), k=2, p=norm)
    want = dk ** 2 if norm == 2 else dk                    # the tree returns the plain Minkowski distance
    assert np.array_equal(i1, ik[:, 0])
    assert np.abs(d1 - want[:, 0]).max() <= 1e-14 and np.abs(d2 - want[:, 1]).max() <= 1e-14
    assert np.array_equal(d1, CO.pair_distance(x, y[i1], norm)) and (d2 >= d1).all()


def test_oracle_hand_case():
    """x = 3 rows, y = 2 rows, by hand.  norm 2 is SQUARED, norm 1 is not."""
    x = np.array([[0, 0, 0], [1, 2, 2], [0.5, 0, 0]], dtype=np.float32)
    y = np.array([[1, 0, 0], [0, 0, -0.25]], dtype=np.float32)
    d1, i1, d2 = CO.nearest(x, y, 2)
    assert i1.tolist() == [1, 0, 0] and d1.tolist() == [0.0625, 8.0, 0.25] and d2.tolist() == [1.0, 10.0625, 0.3125]
    d1, i1, d2 = CO.nearest(x, y, 1)
    assert i1.tolist() == [1, 0, 0] and d1.tolist() == [0.25, 4.0, 0.5] and d2.tolist() == [1.0, 5.25, 0.75]
    # the tie of the first direction's third row under L1 would be 0.5 against 0.75: no tie; an exact tie takes the smaller index
    d1, i1, _ = CO.nearest(np.zeros((1, 3), np.float32), np.array([[0, 1, 0], [1, 0, 0], [0, 0, 1]], np.float32), 2)
    assert i1.tolist() == [0] and d1.tolist() == [1.0]
    # chamfer of the hand case, norm 2: mean(0.0625, 8, 0.25) + mean over y of its nearest x: y0 -> x2 (0.25), y1 -> x0 (0.0625)
    cd, nc = CO.chamfer(x, y, 2)
    assert nc is None and cd == pytest.approx((0.0625 + 8.0 + 0.25) / 3 + (0.25 + 0.0625) / 2, rel=1e-15)
    # normal term: parallel and anti-parallel normals cost 0, orthogonal ones 1; a zero normal is held by eps
    t = CO.normal_term(np.array([[0, 0, 2.0], [0, 0, -1.0], [1.0, 0, 0], [0, 0, 0]]), np.array([[0, 0, 1.0]]), np.zeros(4, int))
    assert t.tolist() == [0.0, 0.0, 1.0, 1.0]


def test_oracle_vertex_normals_hand_case():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 3], [5, 5, 5]], dtype=np.float64)
    f = np.array([[0, 1, 2], [0, 3, 1], [0, 1, 9]])                       # xy triangle (area 1/2), xz triangle (area 3/2), one bad face
    n = CO.vertex_normals(v, f)
    w = np.array([0.0, 3.0, 1.0]) / np.sqrt(10.0)                         # (0,0,1) + (0,3,0): area weighting
    assert np.allclose(n[0], w) and np.allclose(n[1], w) and n[2].tolist() == [0, 0, 1] and np.allclose(n[3], [0, 1, 0])
    assert n[4].tolist() == [0, 0, 1]                                     # unreferenced


def test_workspace_sizes_are_monotone_and_aligned():
    lib = _lib.load()
    for fn in (lib.dudf_nearest_workspace_bytes, lib.dudf_chamfer_terms_workspace_bytes, lib.dudf_vertex_normals_workspace_bytes):
        last = 0
        for n in (0, 1, 31, 32, 33, 1000, 4097, 100000, 1000003, (1 << 31) - 1):
            b = fn(n)
            assert b % 256 == 0 and b >= 256 and b >= last, (n, b, last)
            last = b
    assert lib.dudf_nearest_workspace_bytes(100000) >= 8 * 100000
    assert lib.dudf_vertex_normals_workspace_bytes(100000) >= 24 * 100000


def test_argument_errors_without_a_device():
    lib = _lib.load()
    call = lambda n, m, norm, ws=NULL, nb=0: lib.dudf_nearest_points(NULL, n, NULL, m, norm, NULL, NULL, ws, nb, NULL)  # noqa: E731
    assert call(5, 5, 3) == -3 and call(5, 5, 0) == -3                      # DUDF_E_BADMODE
    assert call(0, 0, 2) == 0 and call(0, 7, 1) == 0                        # n == 0: nothing to do
    assert call(5, 0, 2) == -1 and call(5, -1, 1) == -1                     # DUDF_E_BADCFG
    assert call(1 << 31, 5, 2) == -4 and call(5, 1 << 31, 1) == -4          # DUDF_E_UNSUPPORTED
    # workspace: missing, too small, misaligned (host addresses are never dereferenced: the checks come first)
    buf = ctypes.create_string_buffer(4096 + 512)
    base = (ctypes.addressof(buf) + 255) // 256 * 256
    xs = (ctypes.c_float * 30)()
    ok = lambda ws, nb: lib.dudf_nearest_points(ctypes.cast(xs, ctypes.c_void_p), 10, ctypes.cast(xs, ctypes.c_void_p), 10, 2,  # noqa: E731
                                                NULL, NULL, ctypes.c_void_p(ws), nb, NULL)
    assert ok(0, 0) == -2 and ok(base, 8) == -2 and ok(base + 64, 4096) == -2
    assert lib.dudf_chamfer_terms(NULL, NULL, 5, NULL, NULL, 0, NULL, NULL, 0, NULL) == -1
    assert lib.dudf_vertex_normals(NULL, -1, NULL, 0, NULL, NULL, 0, NULL) == -1
    assert lib.dudf_vertex_normals(NULL, 0, NULL, 0, NULL, NULL, 0, NULL) == 0


def test_cuantitative_imports_without_pytorch3d_or_open3d(tmp_path):
    import cuantitative
    assert "pytorch3d" not in sys.modules and "open3d" not in sys.modules
    assert callable(cuantitative.metrics) and callable(cuantitative.run)
    assert cuantitative.HEADER == "mesh,time,L1CD_CAP,L2CD_CAP,NC_CAP,L1CD_MU,L2CD_MU,NC_MU"
    cfg = cuantitative.default_exp_config("out/")
    assert cfg["num_epochs"] == 3000 and cfg["s1_epochs"] == 2000 and cfg["warmup_epochs"] == 1000 and cfg["resolution"] == 256
    assert cfg["network"]["hidden_layer_nodes"] == [256] * 8 and cfg["checkpoint_path"] == "out/"
    # the cloud holder reads what mesh.py writes
    from diffudf_amd import mesh
    p = np.arange(12, dtype=np.float32).reshape(4, 3); n = np.tile(np.array([0, 0, 1], np.float32), (4, 1))
    mesh.write_ply_points(str(tmp_path / "a_pc.ply"), p, n)
    pc = cuantitative.PointCloudFile(str(tmp_path / "a_pc.ply"))
    assert np.array_equal(pc.points, p) and np.array_equal(pc.normals, n)

    class M:
        vertices = p.astype(np.float64); vertex_normals = n
    with pytest.raises(_lib.DudfError):                                   # no CPU fallback behind the reference's surface either
        cuantitative.metrics(M, pc, 2, "cpu")


def test_run_names_the_experiment_that_gave_no_mesh(tmp_path, monkeypatch):
    """`setup_train` returns an empty mesh list for `resolution` 0 or when no epoch improved: `run` says which experiment."""
    import cuantitative
    import train
    data = tmp_path / "data" / "shirt"; os.makedirs(data)
    (data / "shirt_pc.ply").write_bytes(b""); (data / "shirt_t.obj").write_bytes(b"")
    seen = []
    monkeypatch.setattr(train, "setup_train", lambda cfg, dev: (seen.append(dict(cfg)), (1.5, []))[1])
    with pytest.raises(RuntimeError, match="shirt"):
        cuantitative.run(str(tmp_path / "data"), str(tmp_path / "out"), 0, exp_config=cuantitative.default_exp_config("x"))
    assert seen[0]["experiment_name"] == "shirt" and seen[0]["dataset"] == str(data / "shirt") and seen[0]["checkpoint_path"] == str(tmp_path / "out")
    assert open(tmp_path / "out" / "results.csv").read() == cuantitative.HEADER + "\n"


def test_no_cpu_fallback_and_no_ignored_keywords():
    from diffudf_amd import metrics
    from diffudf_amd.render_mc import TriangleSoup
    a = torch.zeros(4, 3)
    with pytest.raises(_lib.DudfError):
        metrics.chamfer_distance(a, a)
    with pytest.raises(_lib.DudfError):
        metrics.nearest_points(a, a)
    with pytest.raises(_lib.DudfError):
        metrics.vertex_normals(a.double(), torch.zeros(1, 3, dtype=torch.int64))
    for kw in ("point_reduction", "batch_reduction", "x_lengths", "single_directional", "abs_cosine"):
        with pytest.raises(TypeError):
            metrics.chamfer_distance(a, a, **{kw: None})
    assert isinstance(TriangleSoup.vertex_normals, property)
