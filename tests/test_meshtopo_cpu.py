# coding: utf-8
"""CPU: the mesh-topology rules as tests/meshtopo_oracle.py states them — planted meshes with their answers written
out, an independent recount of the same-direction edges on the oracle's output, the welded CAP-UDF soups the device comparison
(tests/test_meshtopo_gpu.py) runs on, and the C ABI's argument checks, which are host arithmetic in front of any device call."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshtopo_oracle as T  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64 = np.int64


def counts(r):
    return tuple(r[k] for k in T.COUNT_NAMES)


def same_direction_edges(f, V):
    """Independent of the oracle's edge table: a manifold edge whose two faces traverse it the same way is a DIRECTED edge with two
    uses whose reverse has none (python dicts over the faces that are not ignored)."""
    uses = {}
    for a, b, c in np.asarray(f, I64).tolist():
        if min(a, b, c) < 0 or max(a, b, c) >= V or a == b or b == c or c == a:
            continue
        for e in ((a, b), (b, c), (c, a)):
            uses[e] = uses.get(e, 0) + 1
    return sum(1 for (a, b), n in uses.items() if n == 2 and (b, a) not in uses)


def manifold_edge_count(f, V):
    und = {}
    for a, b, c in np.asarray(f, I64).tolist():
        if min(a, b, c) < 0 or max(a, b, c) >= V or a == b or b == c or c == a:
            continue
        for e in ((a, b), (b, c), (c, a)):
            k = (min(e), max(e))
            und[k] = und.get(k, 0) + 1
    return sum(1 for n in und.values() if n == 2)


# ---------------------------------------------------------------------------------------------------------------- planted meshes
def test_two_faces_on_one_edge():
    opposite = np.array([[0, 1, 2], [1, 0, 3]])            # 0 -> 1 and 1 -> 0: consistent
    r = T.topology(opposite, 4)
    assert counts(r) == (1, 1, 1, 4, 0, 0, 0, 0)
    assert r["flip"].tolist() == [0, 0] and r["component"].tolist() == [0, 0] and np.array_equal(r["faces"], opposite)
    same = np.array([[0, 1, 2], [0, 1, 3]])                # both 0 -> 1: the second face turns
    r = T.topology(same, 4)
    assert counts(r) == (1, 1, 1, 4, 0, 0, 1, 0)
    assert r["flip"].tolist() == [0, 1] and r["faces"].tolist() == [[0, 1, 2], [0, 3, 1]]
    assert r["component_faces"].tolist() == [2, 0] and r["labels"].tolist() == [0] and r["area"] is None
    # the label face is the smallest index whatever the order: swapped, face 0 = (0,1,3) stays and (0,1,2) turns
    r = T.topology(same[::-1], 4)
    assert r["faces"].tolist() == [[0, 1, 3], [0, 2, 1]]


def test_a_closed_tetrahedron_with_one_face_reversed():
    f = T.TETRA_F.copy()
    f[2] = f[2][[0, 2, 1]]
    r = T.topology(f, 4, T.TETRA_V)
    assert counts(r) == (1, 3, 6, 0, 0, 0, 1, 0)
    assert r["flip"].tolist() == [0, 0, 1, 0] and np.array_equal(r["faces"], T.TETRA_F)
    # areas: three right triangles (nn = 1) and the slanted face (nn = sqrt 3): q = rint(nn * 2^30), area = sum * 2^-31
    q = 3 * 2 ** 30 + int(np.rint(np.sqrt(3.0) * 2 ** 30))
    assert r["area_q"].tolist() == [q] and r["component_area_q"].tolist() == [q, 0, 0, 0]
    assert abs(r["area"][0] - (1.5 + np.sqrt(3.0) / 2)) < 2 ** -29
    # reversing the label face instead turns the three others: the label face keeps ITS winding
    g = T.TETRA_F.copy()
    g[0] = g[0][[0, 2, 1]]
    r = T.topology(g, 4)
    assert r["flip"].tolist() == [0, 1, 1, 1] and r["inconsistent_edges"] == 0


def test_a_moebius_band_has_a_defined_result_and_says_so():
    v, f = T.mobius(12)
    r = T.topology(f, len(v), v)
    assert r["components"] == 1 and r["forest_edges"] == 23 and r["manifold_edges"] == 24 and r["border_edges"] == 24
    assert r["inconsistent_edges"] >= 1
    assert same_direction_edges(r["faces"], len(v)) == r["inconsistent_edges"]
    r2 = T.topology(T.scramble(f, 3), len(v), v)
    assert r2["inconsistent_edges"] >= 1 and r2["components"] == 1
    # the same band without the twist is orientable
    vc, fc = T.mobius(12)
    fc = fc.copy(); n = 12
    fc[-2:] = [[n - 1, 0, 2 * n - 1], [0, n, 2 * n - 1]]
    assert T.topology(T.scramble(fc, 3), len(vc))["inconsistent_edges"] == 0


def test_three_faces_on_one_edge_are_three_components():
    v, f = T.fin()
    r = T.topology(f, len(v), v)
    assert counts(r) == (3, 0, 0, 6, 1, 0, 0, 0)
    assert r["component"].tolist() == [0, 1, 2] and r["flip"].tolist() == [0, 0, 0] and r["n_faces"].tolist() == [1, 1, 1]


def test_a_duplicated_face_shares_three_manifold_edges_with_its_twin():
    r = T.topology(np.array([[0, 1, 2], [0, 1, 2]]), 3)
    assert counts(r) == (1, 1, 3, 0, 0, 0, 1, 0) and r["faces"].tolist() == [[0, 1, 2], [0, 2, 1]]
    r = T.topology(np.array([[0, 1, 2], [1, 0, 2]]), 3)    # the twin already reversed
    assert counts(r) == (1, 1, 3, 0, 0, 0, 0, 0)


def test_ignored_faces():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [np.nan, 0, 0]])
    f = np.array([[0, 5, 1], [0, 1, 2], [2, 2, 3], [2, 1, 3], [-1, 0, 1], [1, 3, 1]])
    r = T.topology(f, 5, v)
    assert r["ignored_faces"] == 4 and r["components"] == 5 and r["manifold_edges"] == 1 and r["border_edges"] == 4
    assert r["component"].tolist() == [0, 1, 2, 1, 4, 5] and r["flip"].tolist() == [0] * 6
    assert np.array_equal(r["faces"], f)
    assert r["component_faces"].tolist() == [1, 2, 1, 0, 1, 1]
    assert r["component_area_q"].tolist() == [0, 2 ** 31, 0, 0, 0, 0]     # ignored faces have no area
    # a non-finite face normal weighs nothing; nn above 16 saturates
    r = T.topology(np.array([[0, 1, 4], [0, 1, 2]]), 5, v * np.array([100.0, 100.0, 1.0]))
    assert r["component_area_q"].tolist() == [2 ** 34, 0] and r["n_faces"].tolist() == [2]
    assert counts(T.topology(np.zeros((0, 3), I64), 0)) == (0,) * 8


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 513])
def test_scrambled_strips_come_out_consistent(n):
    v, f = T.strip(n)
    assert same_direction_edges(f, len(v)) == 0
    g = T.scramble(f, n)
    r = T.topology(g, len(v), v)
    assert counts(r)[:6] == (1, n - 1, n - 1, n + 2, 0, 0) and r["inconsistent_edges"] == 0
    assert same_direction_edges(r["faces"], len(v)) == 0
    assert r["flipped_faces"] == int(r["flip"].sum()) and r["flip"][0] == 0
    assert r["area_q"].tolist() == [n * 2 ** 30]


def test_the_oracle_does_not_certify_itself():
    """inconsistent_edges is recounted from the output faces alone, on meshes that start inconsistent."""
    for seed, (v, f) in enumerate([T.grid_plane(8, 8), T.tetrahedra(20), T.mobius(9), T.strip(40)]):
        g = T.scramble(f, seed)
        before = same_direction_edges(g, len(v))
        r = T.topology(g, len(v), v)
        assert before > 0
        assert same_direction_edges(r["faces"], len(v)) == r["inconsistent_edges"]
        assert manifold_edge_count(g, len(v)) == r["manifold_edges"]
        assert sorted(map(sorted, r["faces"].tolist())) == sorted(map(sorted, g.tolist()))
        if r["inconsistent_edges"] == 0:                   # orienting an oriented mesh flips nothing
            assert T.topology(r["faces"], len(v))["flipped_faces"] == 0
    v, f = T.tetrahedra(20)
    r = T.topology(T.scramble(f, 5, permute=False), len(v), v)
    assert r["components"] == 20 and r["labels"].tolist() == list(range(0, 80, 4)) and r["n_faces"].tolist() == [4] * 20


@pytest.mark.parametrize("kind,n,faces,manifold,same,components,largest", [
    ("sheet", 33, 735, 935, 141, 11, [180, 180, 97, 58, 58]),
    ("sphere", 33, 2278, 3128, 543, 3, [2242, 18, 18]),
    ("sheet", 65, 3571, 4953, 713, 5, [1793, 1664, 44, 44, 26])])
def test_welded_cap_udf_soups_are_inconsistent_until_oriented(kind, n, faces, manifold, same, components, largest):
    """CAP-UDF signs each cell against its own corner 000: about one manifold edge in six of the welded soup is traversed the same
    way by both faces.  These are the meshes the device comparison runs on; it cannot pass on trivially consistent input."""
    v, f = T.cap_welded(kind, n)
    assert len(f) == faces and manifold_edge_count(f, len(v)) == manifold and same_direction_edges(f, len(v)) == same
    r = T.topology(f, len(v), v)
    assert r["manifold_edges"] == manifold and r["components"] == components and r["nonmanifold_edges"] == 0
    assert sorted(r["n_faces"].tolist(), reverse=True)[:5] == largest
    assert r["inconsistent_edges"] == 0 and same_direction_edges(r["faces"], len(v)) == 0
    assert r["flipped_faces"] > 0 and r["forest_edges"] == faces - components


# ------------------------------------------------------------------------------------------------------------ filter and submesh
def test_filter_thresholds_sit_on_the_integers():
    labels, n, q = np.array([0, 4, 9]), np.array([4, 3, 4]), np.array([2 ** 31, 2 ** 30, 2 ** 31], np.uint64)
    F = T.component_filter
    assert F(labels, n, q, min_faces=4).tolist() == [True, False, True]
    assert F(labels, n, q, min_faces=3).tolist() == [True, True, True]
    assert F(labels, n, q, min_area=0.5).tolist() == [True, True, True]                    # ceil(0.5 * 2^31) = 2^30: stays
    assert F(labels, n, q, min_area=0.5 + 2.0 ** -31).tolist() == [True, False, True]      # 2^30 + 1
    assert F(labels, n, q, min_area_ratio=0.2).tolist() == [True, True, True]              # sum 5 * 2^30: threshold 2^30
    assert F(labels, n, q, min_area_ratio=0.2 + 2.0 ** -30).tolist() == [True, False, True]
    assert F(labels, n, q, keep_largest=1).tolist() == [True, False, False]                # a tie: the smaller label
    assert F(labels, n, q, keep_largest=2).tolist() == [True, False, True]
    assert F(labels, np.array([4, 3, 5]), q, keep_largest=1).tolist() == [False, False, True]   # equal area: more faces first
    assert F(labels, n, q, min_faces=4, keep_largest=5).tolist() == [True, False, True]
    assert F(labels, n, q, keep_largest=0).tolist() == [False, False, False]
    from diffudf_amd import meshclean
    for kw in (dict(min_faces=4), dict(min_area=0.5 + 2.0 ** -31), dict(min_area_ratio=0.2 + 2.0 ** -30), dict(keep_largest=1),
               dict(min_faces=3, keep_largest=2)):
        assert meshclean.component_filter(labels, n, q, **kw).tolist() == F(labels, n, q, **kw).tolist(), kw


def test_submesh_keeps_orders_and_reindexes():
    v = np.arange(21, dtype=np.float64).reshape(7, 3)
    f = np.array([[6, 1, 3], [0, 1, 2], [3, 1, 6], [4, 5, 9]])
    vo, fo, c = T.submesh(v, f, [1, 0, 1, 1])
    assert c == (3, 2) and vo.tolist() == v[[1, 3, 6]].tolist() and fo.tolist() == [[2, 0, 1], [1, 0, 2]]
    vo, fo, c = T.submesh(v, f, [0, 0, 0, 0])
    assert c == (0, 0) and vo.shape == (0, 3) and fo.shape == (0, 3)
    tv, tf = T.tetrahedra(3)
    vo, fo, c = T.remove_small_components(tv, np.concatenate([tf, [[0, 1, 4]]]), min_faces=4)     # on a non-manifold edge: its own component
    assert c == (12, 12) and np.array_equal(fo, tf)


# ------------------------------------------------------------------------------------------------------------------------ the C ABI
NEW_SYMBOLS = ("dudf_mesh_topology_workspace_bytes", "dudf_mesh_topology", "dudf_mesh_submesh_workspace_bytes",
               "dudf_mesh_submesh_count", "dudf_mesh_submesh_emit")


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
    from diffudf_amd import hip_ops, meshclean
    assert hip_ops.MESH_TOPOLOGY_COUNTS == T.COUNT_NAMES
    for fn in ("face_topology", "orient_faces", "remove_small_components"):
        assert callable(getattr(meshclean, fn))


def test_c_abi_refuses_bad_arguments_on_the_host():
    from diffudf_amd import _lib
    lib = _lib.load()
    F = 1000
    need = lib.dudf_mesh_topology_workspace_bytes(F)
    # 20 bytes per table slot (cap = 8192 >= 6 F), 37 per face, two 256-byte heads; every array on a 256-byte granule
    r = lambda n: (n + 255) // 256 * 256  # noqa: E731
    cap = 8192
    assert need == 2 * 256 + 2 * r(4 * cap) + r(8 * cap) + r(4 * cap) + 3 * r(4 * F) + r(8 * F) + r(12 * F) + r(F)
    assert lib.dudf_mesh_topology_workspace_bytes(0) > 0 and lib.dudf_mesh_topology_workspace_bytes(-1) == 0
    limit = (1 << 32) // 6 + 1                           # the smallest F with 6 F >= 2^32
    assert 6 * limit >= 1 << 32 and 6 * (limit - 1) < 1 << 32
    assert lib.dudf_mesh_topology_workspace_bytes(limit) == 0 and lib.dudf_mesh_topology_workspace_bytes(limit - 1) > 0
    P = ctypes.c_void_p
    a, b = P(256), P(512)                                # non-null, aligned addresses that no refused call may touch
    big = 1 << 50
    topo = lib.dudf_mesh_topology
    assert topo(a, limit, 10, None, b, b, b, b, b, b, b, big, None) == -4                    # DUDF_E_UNSUPPORTED
    assert topo(a, 10, 1 << 31, None, b, b, b, b, b, b, b, big, None) == -4
    assert topo(a, -1, 10, None, b, b, b, b, b, b, b, big, None) == -1                       # DUDF_E_BADCFG
    assert topo(a, 10, -1, None, b, b, b, b, b, b, b, big, None) == -1
    assert topo(None, 10, 10, None, b, b, b, b, b, b, b, big, None) == -1
    for hole in range(6):                                # every output is required
        outs = [b] * 6
        outs[hole] = None
        assert topo(a, 10, 10, None, *outs, b, big, None) == -1, hole
    assert topo(a, 10, 10, None, a, b, b, b, b, b, b, big, None) == -1                       # oriented faces may not alias the input
    assert topo(a, 10, 10, None, b, b, b, b, b, b, None, big, None) == -2                    # DUDF_E_WORKSPACE
    assert topo(a, 10, 10, None, b, b, b, b, b, b, P(264), big, None) == -2
    assert topo(a, 10, 10, None, b, b, b, b, b, b, b, lib.dudf_mesh_topology_workspace_bytes(10) - 1, None) == -2
    assert topo(None, 0, 0, None, None, None, None, None, None, None, b, big, None) == -1    # F = 0 still needs out_counts
    assert lib.dudf_mesh_submesh_workspace_bytes(1000, 2000) >= 5 * 1000 + 2000 and lib.dudf_mesh_submesh_workspace_bytes(0, 0) > 0
    assert lib.dudf_mesh_submesh_workspace_bytes(1 << 31, 1) == 0 and lib.dudf_mesh_submesh_workspace_bytes(1, 1 << 31) == 0
    cnt, emit = lib.dudf_mesh_submesh_count, lib.dudf_mesh_submesh_emit
    assert cnt(1 << 31, a, 10, a, b, b, big, None) == -4 and cnt(10, a, 1 << 31, a, b, b, big, None) == -4
    assert cnt(-1, a, 10, a, b, b, big, None) == -1 and cnt(10, None, 10, a, b, b, big, None) == -1
    assert cnt(10, a, 10, None, b, b, big, None) == -1 and cnt(10, a, 10, a, None, b, big, None) == -1
    assert cnt(10, a, 10, a, b, None, big, None) == -2 and cnt(10, a, 10, a, b, b, 16, None) == -2
    assert emit(None, 10, a, 10, a, b, b, b, big, None) == -1 and emit(a, 10, a, 10, a, None, b, b, big, None) == -1
    assert emit(a, 10, a, 10, a, b, None, b, big, None) == -1 and emit(a, 10, a, 10, a, b, b, b, 16, None) == -2


def test_finish_keyword_is_checked_before_anything_runs():
    from diffudf_amd import render_mc
    for bad in ("weld", {"min_size": 3}, 1):
        with pytest.raises(ValueError):
            render_mc._finish_soup(None, None, bad)
    import generate_mc
    with pytest.raises(ValueError):
        generate_mc.generate_mc(None, "tanh", "cpu", 8, "x.obj", algorithm="cap", cap_finish="weld")
