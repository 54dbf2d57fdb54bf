# coding: utf-8
"""CPU: the numpy oracle of the K-nearest search and the normal orientation (tests/orient_oracle.py) on clouds whose answer is known,
and the argument checks of the two C entry points (they return before their first HIP call: fake pointers, as in test_cabi_errors.py).

Every cloud gets independently random sign flips from default_rng(0); K = 10."""
import ctypes
import os

import numpy as np
import pytest

import orient_oracle as OO
from diffudf_amd import _lib, mesh

HERE = os.path.dirname(os.path.abspath(__file__))
OK, E_CFG, E_WS, E_MODE, E_UNSUP = 0, -1, -2, -3, -4
K = 10


def run(points, true_normals):
    _, idx = OO.knn(points, points, K, exclude_self=True)
    res = OO.orient(points, OO.random_flips(true_normals), idx)
    assert np.array_equal(np.abs(res["normals"]), np.abs(true_normals))
    assert res["forest_edges"] == len(points) - res["components"]
    return res


@pytest.mark.parametrize("n", [4000, 20000])
def test_sphere_comes_out_outward(n):
    p, nrm = OO.sphere(n)
    res = run(p, nrm)
    assert res["components"] == 1 and (res["component"] == 0).all()
    assert OO.inconsistent(res["normals"], nrm, res["component"]) == 0
    assert ((res["normals"] * p).sum(axis=1) > 0).all()          # the seed is the top of the sphere: +z is outward there


def test_torus_is_one_consistent_component():
    p, nrm = OO.torus(20000)
    res = run(p, nrm)
    assert res["components"] == 1
    assert OO.inconsistent(res["normals"], nrm, res["component"]) == 0


def test_two_spheres_are_seeded_separately():
    p, nrm = OO.two_spheres(3000)
    res = run(p, nrm)
    assert res["components"] == 2 and res["forest_edges"] == 5998
    assert set(np.unique(res["component"]).tolist()) == {0, 3000}
    assert np.array_equal(res["normals"], nrm)                    # each sphere outward: its own top point decides


def test_beetle():
    """20 000 area-uniform points of the normalised beetle with their triangle normals.  Measured: one component and 195 normals that
    disagree with the triangle normals up to the global sign (thin parts and creases, where the 10 nearest neighbours include the
    opposite sheet).  The bound is 400 — a guard on the rule, not a precision claim."""
    v, t = mesh.load_obj(os.path.join(HERE, "golden", "beetle.obj"))
    p, nrm = mesh.sample_surface(mesh.normalize_vertices(v), t, 20000, seed=1)
    p, nrm = p.astype(np.float32), nrm.astype(np.float32)
    res = run(p, nrm)
    bad = OO.inconsistent(res["normals"], nrm, res["component"])
    print(f"beetle: {res['components']} component(s), {bad} inconsistent normals")
    assert res["components"] == 1
    assert bad <= 400


def test_knn_oracle_orders_ties_by_index_and_pads():
    y = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [np.nan, 0, 0]], dtype=np.float32)
    d, i = OO.knn(y[:1], y, 4)
    assert i.tolist() == [[0, 1, 2, 3]] and d.tolist() == [[0.0, 1.0, 1.0, 1.0]]
    d, i = OO.knn(y[:4], y[:4], 4, exclude_self=True)
    assert i[0].tolist() == [1, 2, 3, -1] and d[0, 3] == np.inf
    big = np.random.default_rng(5).random((5000, 3)).astype(np.float32)         # the candidate path agrees with the exact one
    d1, i1 = OO.knn(big[:300], big, 7, exclude_self=True)
    dd = ((big[:300, None, :].astype(np.float64) - big[None, :, :].astype(np.float64)) ** 2).sum(axis=2)
    dd[np.arange(300), np.arange(300)] = np.inf
    i2 = np.argsort(dd, axis=1, kind="stable")[:, :7]
    assert np.array_equal(i1, i2) and np.array_equal(d1, np.take_along_axis(dd, i2, axis=1))


def test_orient_oracle_ignores_bad_slots_and_breaks_ties_by_slot():
    p = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [9, 9, 9]], dtype=np.float32)
    nrm = np.array([[0, 0, -1], [0, 0, 1], [0, 0, -1], [0, 0, -1]], dtype=np.float32)
    idx = np.array([[1, -1], [0, 2], [1, 2], [3, 7]], dtype=np.int64)          # -1, a self entry, an index past n
    res = OO.orient(p, nrm, idx)
    assert res["components"] == 2 and res["forest_edges"] == 2
    assert res["component"].tolist() == [0, 0, 0, 3]
    assert res["flip"].tolist() == [1, 0, 1, 1]                   # seed of {0,1,2}: vertex 0 (equal z, smallest index), n_z < 0


# ---- the C entry points ------------------------------------------------------------------------------------------------------------
_arena = ctypes.create_string_buffer(1 << 22)
BASE = (ctypes.addressof(_arena) + 255) // 256 * 256
P = ctypes.c_void_p(BASE)
N = 8


def test_symbols_are_exported():
    lib = _lib.load()
    for name in ("dudf_knn_workspace_bytes", "dudf_knn_grid_build", "dudf_knn_points", "dudf_orient_workspace_bytes", "dudf_orient_normals"):
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert lib.dudf_abi_version() == 8


@pytest.mark.parametrize("mode", [0, 1])
def test_knn_argument_precedence(mode):
    lib = _lib.load()
    nb = int(lib.dudf_knn_workspace_bytes(N, 4, 3, mode))
    assert 0 < nb <= (1 << 22) - 512
    knn = lambda n, m, k, ws, nbytes=nb, md=mode, x=P: lib.dudf_knn_points(x, n, P, m, k, 0, md, P, P, ws, nbytes, None)  # noqa: E731
    assert knn(N, 4, 3, None, md=2) == E_MODE                     # the mode first
    assert knn(-1, 4, 0, None, md=-1) == E_MODE
    assert knn(-1, 4, 0, None) == E_CFG                           # a negative count before K
    assert knn(N, 4, 0, None) == E_UNSUP
    assert knn(N, 4, 17, None) == E_UNSUP
    assert knn(1 << 31, 4, 3, None) == E_UNSUP
    assert knn(N, 1 << 31, 3, None) == E_UNSUP
    assert knn(0, 4, 17, None) == E_UNSUP                         # K before the empty call
    assert knn(0, 4, 3, None) == OK                               # n == 0: nothing is launched
    assert knn(N, 0, 3, None) == E_CFG                            # the sets before the workspace
    assert knn(N, 4, 3, None, x=None) == E_CFG
    assert knn(N, 4, 3, None) == E_WS
    assert knn(N, 4, 3, ctypes.c_void_p(BASE + 8)) == E_WS
    assert knn(N, 4, 3, P, nb - 1) == E_WS
    assert lib.dudf_knn_workspace_bytes(N, 4, 0, mode) == 0 and lib.dudf_knn_workspace_bytes(N, 4, 17, mode) == 0
    assert lib.dudf_knn_workspace_bytes(-1, 4, 3, mode) == 0 and lib.dudf_knn_workspace_bytes(N, 4, 3, 2) == 0
    assert lib.dudf_knn_grid_build(P, 0, P, nb, None) == E_CFG
    assert lib.dudf_knn_grid_build(None, 4, P, nb, None) == E_CFG
    assert lib.dudf_knn_grid_build(P, 1 << 31, P, nb, None) == E_UNSUP
    assert lib.dudf_knn_grid_build(P, 4, None, nb, None) == E_WS


def test_orient_argument_precedence():
    lib = _lib.load()
    nb = int(lib.dudf_orient_workspace_bytes(N, 3))
    assert 0 < nb <= (1 << 22) - 512
    ori = lambda n, k, ws, nbytes=nb, pts=P, nrm=P, idx=P: lib.dudf_orient_normals(pts, nrm, idx, n, k, P, P, P, P, None, ws, nbytes, None)  # noqa: E731
    assert ori(-1, 0, None) == E_CFG
    assert ori(N, 0, None) == E_UNSUP
    assert ori(N, 17, None) == E_UNSUP
    assert ori(1 << 31, 1, None) == E_UNSUP
    assert ori(1 << 30, 4, None) == E_UNSUP                       # n * K = 2^32 slots
    assert ori((1 << 28) - 1, 16, None) == E_WS                   # ... one vertex fewer: the slots fit, the workspace does not
    assert ori(0, 3, None) == OK
    assert ori(N, 3, None, pts=None) == E_CFG                     # the inputs before the workspace
    assert ori(N, 3, None, nrm=None) == E_CFG
    assert ori(N, 3, None, idx=None) == E_CFG
    assert ori(N, 3, None) == E_WS
    assert ori(N, 3, ctypes.c_void_p(BASE + 8)) == E_WS
    assert ori(N, 3, P, nb - 1) == E_WS
    assert lib.dudf_orient_workspace_bytes(1 << 30, 4) == 0 and lib.dudf_orient_workspace_bytes(N, 0) == 0
    stats = (ctypes.c_int64 * 2)(7, 7)
    assert lib.dudf_orient_normals(P, P, P, 0, 3, P, P, P, P, stats, None, 0, None) == OK and list(stats) == [0, 0]


def test_generate_pc_point_cloud_has_the_method():
    import generate_pc
    assert callable(getattr(generate_pc.PointCloud, "orient_normals_consistent_tangent_plane"))
