# coding: utf-8
"""CPU: the mesh-simplification rules as tests/simplify_oracle.py states them — the oracle against itself on a
lattice plane whose answer can be written out, planted defects with their counts, the share of cells whose decisions sit on a threshold
for every input of the device comparison (tests/test_simplify_gpu.py), the C ABI's argument checks, which are host arithmetic in front
of any device call, and the export list."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshtopo_oracle as T  # noqa: E402
import simplify_oracle as S  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------ the oracle against itself
def plane(w_b, grid=8):
    v, f = T.grid_plane(64, 64)
    h = S.extent(v) / grid
    r = S.simplify(v, f, S.centred_origin(v, h), h, w_b)
    bv = S.border_vertices(r["faces"], len(r["vertices"]))
    p = r["vertices"][bv]
    off = np.minimum(np.minimum(np.abs(p[:, 0]), np.abs(p[:, 0] - 1)), np.minimum(np.abs(p[:, 1]), np.abs(p[:, 1] - 1)))
    return r, h, off


def test_a_lattice_plane_keeps_its_plane_and_its_border():
    """grid_plane(64, 64) at grid 8, the lattice centred on the border (`centred_origin`: with the origin ON the bounding-box minimum the
    plane and its border lie on cell faces, every minimiser sits at |x_d| = 0.5 and the containment test of rule 7 is decided by
    rounding): 9 x 9 cells, 8 x 8 x 2 = 128 faces, the plane kept to rounding and, with w_b = 1, the border kept too."""
    r, h, off = plane(1.0)
    c = r["counts"]
    assert (c["vertices"], c["faces"], c["cells"], c["invalid"], c["duplicate"], c["border_edges"], c["fallback"]) == (81, 128, 81, 0, 0, 256, 0)
    assert c["collapsed"] == 8192 - 128
    assert sorted(map(tuple, np.rint(r["vertices"][:, :2] * 8).astype(int).tolist())) == [(i, j) for i in range(9) for j in range(9)]
    print(f"plane: max |z| {np.abs(r['vertices'][:, 2]).max() / h:.3e} h, border vertices off the border by at most {off.max() / h:.3e} h")
    assert np.abs(r["vertices"][:, 2]).max() <= 1e-12 * h
    assert len(off) == 32 and off.max() <= 1e-9 * h
    # the surviving faces are distinct and wound as the input (+z); interior vertices sit at xhat, so the areas vary
    p = r["vertices"][r["faces"]]
    nz = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])[:, 2]
    assert (nz > 0).all() and abs(nz.sum() - 2.0) < 1e-12 and len(set(map(tuple, np.sort(r["faces"], 1).tolist()))) == 128


def test_without_the_border_term_the_border_erodes():
    r, h, off = plane(0.0)
    print(f"plane, w_b = 0: border vertices off the border by up to {off.max() / h:.3f} h")
    assert r["counts"]["faces"] == 128 and np.abs(r["vertices"][:, 2]).max() <= 1e-12 * h
    assert off.max() > 0.1 * h


def test_planted_defects_are_counted():
    v, f, facts = S.planted()
    for w in (0.0, 1.0):
        r = S.simplify(v, f, S.PLANTED_ORIGIN, S.PLANTED_H, w)
        c = r["counts"]
        assert c["invalid"] == facts["invalid"] and c["duplicate"] == facts["duplicate"]
        assert facts["corner_key"] in r["cell_keys"].tolist()               # floor() of a dyadic coordinate on a cell corner: that cell
        assert all(k in r["cell_keys"].tolist() for k in facts["saturated_keys"])    # x = 1e7 -> 2^21 - 1, y = -5 -> 0
        assert np.isfinite(r["vertices"]).all() and c["vertices"] == len(r["vertices"]) and c["faces"] == len(r["faces"])
    # the second face over the cell triple goes, the first keeps its winding
    a = S.simplify(v, np.delete(f, facts["first_duplicate"] + 1, 0), S.PLANTED_ORIGIN, S.PLANTED_H)
    b = S.simplify(v, f, S.PLANTED_ORIGIN, S.PLANTED_H)
    assert np.array_equal(a["faces"], b["faces"]) and a["counts"]["duplicate"] == 0
    # a repeated index counts as collapsed, not invalid; a non-manifold edge is no border edge
    one = S.simplify(np.eye(3), [[0, 0, 1]], np.full(3, -0.5), 0.4)["counts"]
    assert (one["collapsed"], one["invalid"], one["cells"]) == (1, 0, 0)
    fv, ff = T.fin()
    fin = S.simplify(fv, ff, np.full(3, -1.25), 0.5)["counts"]
    assert fin["border_edges"] == 6 and fin["faces"] == 3
    empty = S.simplify(np.zeros((0, 3)), np.zeros((0, 3), np.int64), np.zeros(3), 1.0)
    assert set(empty["counts"].values()) == {0} and empty["vertices"].shape == (0, 3) and empty["faces"].shape == (0, 3)


def test_records_follow_face_order_and_sums_follow_records():
    """Two faces in one cell with the third: the sum is ((0 + q_0) + q_1), and permuting the faces changes which comes first."""
    rng = np.random.default_rng(3)
    v = rng.random((5, 3)) * 0.2 + np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0, 0, 0]])
    f = np.array([[0, 1, 2], [4, 3, 1]])
    r = S.simplify(v, f, np.full(3, -0.25), 0.5, 0.0)
    cell0 = 0
    assert r["records"].tolist()[cell0] == 2
    u = (v[f] - (np.full(3, -0.25) + 0.25)) / 0.5
    q = []
    for t in u:
        n = np.cross(t[1] - t[0], t[2] - t[0]); d = -np.dot(n, t[0])
        q.append(np.array([n[0] * n[0], n[0] * n[1], n[0] * n[2], n[1] * n[1], n[1] * n[2], n[2] * n[2], d * n[0], d * n[1], d * n[2], d * d]))
    assert np.allclose(r["quadrics"][cell0], q[0] + q[1], rtol=1e-13, atol=0)
    assert np.allclose(r["xhat"][cell0], (u[0][0] + u[1][0]) / 2, rtol=1e-14)


# ------------------------------------------------------------------------------------------------------------------- decision margins
def test_few_cells_of_the_device_inputs_sit_on_a_threshold():
    """The device comparison holds positions and fallbacks to the oracle only where no decision of rule 7 sits within 1e-8 of its
    threshold; this caps the share of the other cells at 2 % for every input it runs on."""
    worst = 0.0
    for name, (v, f, origin, h, weights) in S.inputs().items():
        for w in weights:
            r = S.result(name, w)
            C = r["counts"]["cells"]
            low = int((r["margin"] < 1e-8).sum())
            share = low / C if C else 0.0
            print(f"{name:28s} w_b = {w}: {low} of {C} cells below the margin ({share:.2%})")
            worst = max(worst, share)
            assert share <= 0.02, (name, w, low, C)
    print(f"worst share {worst:.2%}")


# ------------------------------------------------------------------------------------------------------------------------ the C ABI
NEW_SYMBOLS = ("dudf_mesh_simplify_workspace_bytes", "dudf_mesh_simplify_keys", "dudf_mesh_simplify_count", "dudf_mesh_simplify_emit")


def test_header_binding_and_abi():
    from diffudf_amd import _lib
    src = open(os.path.join(REPO, "include", "dudf_hip.h")).read()
    assert re.search(r"#define DUDF_ABI_VERSION 8\b", src) and _lib.ABI_VERSION == 8
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    assert lib.dudf_abi_version() == 8
    for name in NEW_SYMBOLS:
        decl = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", src)
        assert decl, name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
        assert len(_lib.SYMBOLS[name][1]) == decl.group(1).count(",") + 1, name
    from diffudf_amd import hip_ops, meshclean, render_mc
    assert hip_ops.MESH_SIMPLIFY_COUNTS == S.COUNT_NAMES
    assert callable(meshclean.simplify_mesh) and callable(hip_ops.mesh_simplify) and callable(hip_ops.mesh_simplify_count)
    assert "simplify" in render_mc._FINISH_KEYS


def test_c_abi_refuses_bad_arguments_on_the_host():
    from diffudf_amd import _lib
    lib = _lib.load()
    wsb = lib.dudf_mesh_simplify_workspace_bytes
    assert wsb(1000, 2000) > 0 and wsb(1000, 2000) % 256 == 0 and wsb(0, 0) > 0 and wsb(0, 0) % 256 == 0 and wsb(7, 3) % 256 == 0
    limit = (1 << 31) // 3 + 1                           # the smallest F with 3 F >= 2^31
    assert 3 * limit >= 1 << 31 and 3 * (limit - 1) < 1 << 31
    assert wsb(10, limit) == 0 and wsb(10, limit - 1) > 0 and wsb(1 << 31, 10) == 0 and wsb((1 << 31) - 1, 10) > 0
    assert wsb(-1, 10) == 0 and wsb(10, -1) == 0
    P = ctypes.c_void_p
    a, b = P(256), P(512)                                # non-null, aligned addresses that no refused call may touch
    big = 1 << 50
    org = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    nan, inf = float("nan"), float("inf")
    keys, cnt, emit = lib.dudf_mesh_simplify_keys, lib.dudf_mesh_simplify_count, lib.dudf_mesh_simplify_emit
    BADCFG, WORKSPACE, UNSUPPORTED = -1, -2, -4
    # keys
    assert keys(a, 10, a, limit, org, 0.5, b, b, big, None) == UNSUPPORTED and keys(a, 1 << 31, a, 10, org, 0.5, b, b, big, None) == UNSUPPORTED
    for h in (0.0, -1.0, nan, inf, 1e-320):
        assert keys(a, 10, a, 10, org, h, b, b, big, None) == BADCFG, h
    assert keys(a, 10, a, 10, None, 0.5, b, b, big, None) == BADCFG
    assert keys(a, 10, a, 10, (ctypes.c_double * 3)(0.0, nan, 0.0), 0.5, b, b, big, None) == BADCFG
    assert keys(None, 10, a, 10, org, 0.5, b, b, big, None) == BADCFG and keys(a, 10, None, 10, org, 0.5, b, b, big, None) == BADCFG
    assert keys(a, 10, a, 10, org, 0.5, None, b, big, None) == BADCFG and keys(a, -1, a, 10, org, 0.5, b, b, big, None) == BADCFG
    assert keys(a, 10, a, -1, org, 0.5, b, b, big, None) == BADCFG
    assert keys(a, 10, a, 10, org, 0.5, b, None, big, None) == WORKSPACE and keys(a, 10, a, 10, org, 0.5, b, P(264), big, None) == WORKSPACE
    assert keys(a, 10, a, 10, org, 0.5, b, b, wsb(10, 10) - 1, None) == WORKSPACE
    # count
    ok = (org, 0.5, 1.0, 1e-3, a, a, 1)
    assert cnt(a, 10, a, limit, *ok, b, b, big, None) == UNSUPPORTED and cnt(a, 1 << 31, a, 10, *ok, b, b, big, None) == UNSUPPORTED
    for h in (0.0, -1.0, nan, inf):
        assert cnt(a, 10, a, 10, org, h, 1.0, 1e-3, a, a, 1, b, b, big, None) == BADCFG, h
    for w in (-1e-9, -1.0, nan):
        assert cnt(a, 10, a, 10, org, 0.5, w, 1e-3, a, a, 1, b, b, big, None) == BADCFG, w
    for tau in (0.0, 1.0, -0.5, 2.0, nan):
        assert cnt(a, 10, a, 10, org, 0.5, 1.0, tau, a, a, 1, b, b, big, None) == BADCFG, tau
    assert cnt(a, 10, a, 10, org, 0.5, 1.0, 1e-3, None, a, 1, b, b, big, None) == BADCFG
    assert cnt(a, 10, a, 10, org, 0.5, 1.0, 1e-3, a, None, 1, b, b, big, None) == BADCFG
    assert cnt(a, 10, a, 10, org, 0.5, 1.0, 1e-3, a, a, 2, b, b, big, None) == BADCFG
    assert cnt(a, 10, a, 10, *ok, None, b, big, None) == BADCFG and cnt(None, 10, a, 10, *ok, b, b, big, None) == BADCFG
    assert cnt(a, 10, None, 10, *ok, b, b, big, None) == BADCFG and cnt(a, 10, a, 10, None, *ok[1:], b, b, big, None) == BADCFG
    assert cnt(a, 10, a, 10, *ok, b, None, big, None) == WORKSPACE and cnt(a, 10, a, 10, *ok, b, b, 16, None) == WORKSPACE
    assert cnt(None, 0, None, 0, *ok, None, b, big, None) == BADCFG                           # F = 0 still needs out_counts
    # emit
    assert emit(a, 10, a, limit, b, b, None, None, None, None, None, b, big, None) == UNSUPPORTED
    assert emit(a, 10, a, 10, None, b, None, None, None, None, None, b, big, None) == BADCFG
    assert emit(a, 10, a, 10, b, None, None, None, None, None, None, b, big, None) == BADCFG
    assert emit(a, 10, a, 10, b, b, b, None, b, b, b, b, big, None) == BADCFG                  # the optional outputs: all five or none
    assert emit(a, 10, a, 10, b, b, b, b, b, b, None, b, big, None) == BADCFG
    assert emit(None, 10, a, 10, b, b, None, None, None, None, None, b, big, None) == BADCFG
    assert emit(a, 10, a, 10, b, b, None, None, None, None, None, None, big, None) == WORKSPACE
    assert emit(a, 10, a, 10, b, b, None, None, None, None, None, b, 16, None) == WORKSPACE


def test_keywords_are_checked_before_anything_runs():
    from diffudf_amd import meshclean, render_mc
    for kw in ({}, {"grid": 8, "cell": 0.1}, {"grid": 8, "target_faces": 10}):
        with pytest.raises(ValueError):
            meshclean.simplify_mesh(np.zeros((3, 3)), np.zeros((1, 3), np.int64), **kw)
    for bad in ({"simplify": 8}, {"simplify": {"faces": 10}}):
        with pytest.raises(ValueError):
            render_mc._finish_soup(None, None, bad)
    import generate_mc
    with pytest.raises(ValueError):
        generate_mc.generate_mc(None, "tanh", "cpu", 8, "x.obj", algorithm="cap", simplify_target_faces=10, simplify_grid=4)
    with pytest.raises(ValueError):
        generate_mc.generate_mc(None, "tanh", "cpu", 8, "x.obj", algorithm="cap", simplify_boundary_weight=2.0)
