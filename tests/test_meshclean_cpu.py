# coding: utf-8
"""CPU: the mesh clean-up rules (DESIGN.md §3 "Mesh clean-up") as tests/meshclean_oracle.py states them — hand-built cases with
their answers written out, properties on the MeshUDF outputs of the project's fixtures (the meshes tests/test_meshclean_gpu.py
compares the device on), and the `clean=` keyword of `extract_mesh_MESHUDF` where no device is involved."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshclean_oracle as O  # noqa: E402
from test_meshudf import G10, LUTS, random_fields  # noqa: E402

F64, I64 = np.float64, np.int64
_MESHES = {}


def fixture_meshes():
    """{name: (vertices float64, faces int64)}: the raw `extract_mesh_MESHUDF` output (host library, the fixture's tables) of the 7
    g10 cases and the 40 `random_fields()`; extracted once per session."""
    if not _MESHES:
        from src.render_mc import extract_mesh_MESHUDF
        fields = [(str(t), G10[str(t) + "_udf"], G10[str(t) + "_grads"]) for t in G10["cases"]]
        fields += [(f"random_{trial}", udf, gg) for trial, udf, gg, _ in random_fields()]
        for name, udf, gg in fields:
            _, _, mesh = extract_mesh_MESHUDF(udf, gg, "cpu", luts=LUTS, clean=False)
            _MESHES[name] = (np.asarray(mesh.vertices, F64), np.asarray(mesh.faces, I64))
    return _MESHES


def directed_edge_counts(f):
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    return np.unique(e, axis=0, return_counts=True)


def same_mesh(a, b):
    return a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and a[0].shape == b[0].shape


# ------------------------------------------------------------------------------------------------------------- hand-built cases
def test_a_soup_of_two_triangles_welds_to_four_vertices():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], F64)
    vo, fo, c = O.round(v, np.arange(6).reshape(2, 3))
    assert vo.tolist() == [[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]]
    assert fo.tolist() == [[0, 1, 2], [1, 3, 2]]
    assert (c["vertices"], c["faces"], c["welded"], c["unreferenced"]) == (4, 2, 2, 0)


def test_weld_tolerance_and_the_representative():
    # 4e-9 apart: keys rint(0.4) = rint(0) -> merge into the smaller index, which keeps ITS coordinates; 2e-8 apart: keys 0 and 2
    v = np.array([[5, 5, 5], [0, 0, 4e-9], [1, 0, 0], [0, 1, 0], [0, 0, 0], [0, 0, 2e-8]], F64)
    f = np.array([[4, 2, 3], [1, 3, 0], [5, 0, 2]])
    vo, fo, c = O.round(v, f)
    assert c["welded"] == 1 and c["vertices"] == 5
    assert vo.tolist() == [[5, 5, 5], [0, 0, 4e-9], [1, 0, 0], [0, 1, 0], [0, 0, 2e-8]]
    assert fo.tolist() == [[1, 2, 3], [1, 3, 0], [4, 0, 2]]
    # half to even (exact halves need a scale that keeps them exact: digits = 0 and 1)
    assert O.vertex_keys(np.array([[0.5, 1.5, -0.5], [2.5, -1.5, 3.5]]), digits=0).tolist() == [[0, 2, 0], [2, -2, 4]]
    assert O.vertex_keys(np.array([[0.25, 0.75, -0.25]]), digits=1).tolist() == [[2, 8, -2]]


def test_signed_zero_keys_are_one_key():
    v = np.array([[0.0, 1, 0], [1, 0, 0], [0, 0, 1], [-0.0, 1, -0.0], [-1e-9, 1, 1e-9]], F64)
    vo, fo, c = O.round(v, np.array([[0, 1, 2], [3, 2, 1], [4, 1, 2]]))
    assert O.vertex_keys(v[[0, 3, 4]]).tolist() == [[0, 100000000, 0]] * 3
    assert c["welded"] == 2 and c["duplicate_faces"] == 2 and fo.tolist() == [[0, 1, 2]]
    assert np.signbit(vo[0]).tolist() == [False, False, False]                     # vertex 0's own coordinates


def test_degenerate_and_duplicate_faces_go():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.5, 1e-9, 0], [2, 2, 2], [3, 2, 2], [2, 3, 2]], F64)
    f = np.array([[0, 1, 2],       # kept
                  [0, 0, 1],       # a repeated index
                  [0, 1, 3],       # a sliver of height 1e-9
                  [1, 2, 0],       # duplicate, rotated
                  [2, 1, 0],       # duplicate, reversed
                  [4, 5, 6]])      # kept
    rep, g, state = O.round_parts(v, f)
    assert state.tolist() == [3, 1, 1, 2, 2, 3]
    vo, fo, c = O.round(v, f)
    assert (c["degenerate_faces"], c["duplicate_faces"], c["unreferenced"], c["faces"]) == (2, 2, 1, 2)
    assert fo.tolist() == [[0, 1, 2], [3, 4, 5]] and len(vo) == 6
    # the two thresholds: L <= 1e-8 (a tiny but well-shaped face), height exactly above
    tiny = np.array([[0, 0, 0], [5e-9, 0, 0], [0, 5e-9, 0]], F64)
    assert O.degenerate(tiny[:1], tiny[1:2], tiny[2:]).tolist() == [True]
    ok = np.array([[0, 0, 0], [1, 0, 0], [0.5, 2e-8, 0]], F64)
    assert O.degenerate(ok[:1], ok[1:2], ok[2:]).tolist() == [False]


def test_unreferenced_vertices_go_and_order_stays():
    v = np.array([[9, 9, 9], [0, 0, 0], [8, 8, 8], [1, 0, 0], [0, 1, 0], [7, 7, 7]], F64)
    vo, fo, c = O.round(v, np.array([[4, 1, 3]]))
    assert vo.tolist() == [[0, 0, 0], [1, 0, 0], [0, 1, 0]] and fo.tolist() == [[2, 0, 1]] and c["unreferenced"] == 3


def test_invalid_faces_are_dropped_and_counted():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0], [0, np.inf, 0]], F64)
    f = np.array([[0, 1, 2], [0, 1, 5], [-1, 1, 2], [0, 1, 3], [4, 1, 2]])
    vo, fo, c = O.round(v, f)
    assert c["invalid_faces"] == 4 and fo.tolist() == [[0, 1, 2]] and len(vo) == 3 and c["unreferenced"] == 2


TETRA_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F64)
TETRA_F = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]])          # outward


@pytest.mark.parametrize("missing", range(4))
def test_a_tetrahedron_minus_one_face_is_closed_with_the_right_winding(missing):
    f = np.delete(TETRA_F, missing, axis=0)
    vo, fo, c = O.round_fill(TETRA_V, f)
    assert (c["holes3"], c["holes4"], c["faces"]) == (1, 0, 4)
    assert np.array_equal(fo[:3], f)
    e, n = directed_edge_counts(fo)
    assert len(e) == 12 and (n == 1).all()                                   # every directed edge once: closed and consistently wound
    assert sorted(np.roll(fo[3], -int(np.argmin(fo[3]))).tolist()) == sorted(TETRA_F[missing].tolist())
    assert np.roll(fo[3], -int(np.argmin(fo[3]))).tolist() == np.roll(TETRA_F[missing], -int(np.argmin(TETRA_F[missing]))).tolist()
    assert same_mesh(O.fill_holes(TETRA_V, f), (TETRA_V, fo))


def test_an_octahedron_minus_two_adjacent_faces_gets_a_4_hole_and_two_faces():
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F64)
    full = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
    f = full[2:]                                                              # the hole 0-2-1-4 (the two faces shared the edge 2-4)
    vo, fo, c = O.round_fill(v, f)
    assert (c["holes3"], c["holes4"], c["faces"]) == (0, 1, 8)
    # a = 0, its border neighbours b = 2 < d = 4, c = 1; face 4 runs 2 -> 0, nothing runs 0 -> 2: not reversed
    assert fo[6:].tolist() == [[0, 2, 1], [1, 4, 0]]
    e, n = directed_edge_counts(fo)
    assert len(e) == 24 and (n == 1).all()
    # the mirrored octahedron: now a face runs 0 -> 2 and the new faces are reversed
    vo, fo, c = O.round_fill(v, f[:, ::-1])
    assert fo[6:].tolist() == [[1, 2, 0], [0, 4, 1]]
    e, n = directed_edge_counts(fo)
    assert (n == 1).all()


def test_a_5_hole_is_left_alone():
    k = 5
    ring = np.array([[np.cos(2 * np.pi * i / k), np.sin(2 * np.pi * i / k), 0] for i in range(k)])
    v = np.concatenate([ring, [[0, 0, 1]]])
    f = np.array([[i, (i + 1) % k, k] for i in range(k)])                     # a cone over a pentagon: its base is a 5-hole
    vo, fo, c = O.round_fill(v, f)
    assert (c["holes3"], c["holes4"]) == (0, 0) and np.array_equal(fo, f)
    assert len(O.border_edges(f, len(v))) == 5


def test_a_hole_through_a_busy_vertex_is_left_alone():
    # two open triangles' worth of border meet in vertex 0: it lies on four border edges, so neither 3-cycle is a whole component
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F64)
    f = np.array([[0, 1, 5], [1, 2, 5], [2, 0, 5], [0, 3, 6], [3, 4, 6], [4, 0, 6]])   # two cones; bases 0-1-2 and 0-3-4 open
    e = O.border_edges(f, len(v))
    assert e.tolist() == [[0, 1], [0, 2], [0, 3], [0, 4], [1, 2], [3, 4]]
    vo, fo, c = O.round_fill(v, f)
    assert (c["holes3"], c["holes4"]) == (0, 0) and np.array_equal(fo, f)
    # without the second cone the base is a plain 3-hole
    assert O.round_fill(v, f[:3])[2]["holes3"] == 1


def test_border_smoothing_sums_the_neighbours_in_ascending_order():
    # vertex 3 has the border neighbours 0, 1, 2 (three fins around it, each a single triangle with an own apex); the coordinates
    # make the order of the sum visible: (1e16 + 1) + -1e16 = 0 in double, 1e16 + -1e16 + 1 = 1
    v = np.array([[1e16, 0, 0], [1.0, 0, 0], [-1e16, 0, 0], [0, 0, 0], [0, 5, 0], [0, 6, 0], [0, 7, 0]], F64)
    f = np.array([[3, 0, 4], [3, 1, 5], [3, 2, 6]])
    e = O.border_edges(f, len(v))
    assert [w for u, w in e.tolist() if u == 3] + [u for u, w in e.tolist() if w == 3] == [4, 5, 6, 0, 1, 2]
    out = O.smooth(v, f, iterations=1, lam=0.3)
    # neighbours of 3 ascending: 0, 1, 2, 4, 5, 6
    s = 0.0
    for w in (0, 1, 2, 4, 5, 6):
        s = s + v[w, 0]
    assert s == 0.0 and out[3, 0] == 0.0 + 0.3 * (s / 6.0 - 0.0)
    sy = ((((0.0 + 0.0) + 0.0) + 0.0) + 5.0 + 6.0) + 7.0
    assert out[3, 1] == 0.0 + 0.3 * (sy / 6.0 - 0.0)
    # Jacobi: vertex 4 (neighbours 0 and 3) averages the positions BEFORE the iteration
    assert out[4, 1] == 5.0 + 0.3 * ((0.0 + 0.0 + 0.0) / 2.0 - 5.0)
    two = O.smooth(v, f, iterations=2, lam=0.3)
    assert two.tobytes() == O.smooth(out, f, iterations=1, lam=0.3).tobytes()
    closed = O.smooth(TETRA_V, TETRA_F)
    assert closed.tobytes() == TETRA_V.tobytes()                                 # no border: nothing moves


def test_clean_runs_rounds_until_the_sizes_stop_changing():
    f = np.delete(TETRA_F, 0, axis=0)
    soup_v = TETRA_V[f].reshape(-1, 3); soup_f = np.arange(9).reshape(3, 3)
    vo, fo, info = O.clean(soup_v, soup_f)
    assert (len(vo), len(fo), info["welded"], info["holes3"], info["rounds"]) == (4, 4, 5, 1, 2)
    vo2, fo2, info2 = O.clean(soup_v, soup_f, fill=False)
    assert len(fo2) == 3 and info2["holes3"] == 0


# ------------------------------------------------------------------------------------- properties on the MeshUDF outputs of the fixtures
def test_the_fixture_meshes_hold_every_defect():
    """What DESIGN.md §3 says of the raw extraction, asserted: the device comparison cannot pass on trivial inputs."""
    seen = dict(welded=0, duplicate_faces=0, degenerate_faces=0, holes3=0, holes4=0, busy_border=0, meshes_with_duplicates=0)
    meshes = fixture_meshes()
    assert len(meshes) == 47
    for name, (v, f) in meshes.items():
        c = O.round_fill(v, f)[2]
        for k in ("welded", "duplicate_faces", "degenerate_faces", "holes3", "holes4"):
            seen[k] += c[k]
        seen["meshes_with_duplicates"] += c["welded"] > 0
        vo, fo, _ = O.clean(v, f)
        e = O.border_edges(fo, len(vo))
        seen["busy_border"] += int(len(e) and np.bincount(e.reshape(-1)).max() > 2)
    assert all(n > 0 for n in seen.values()), seen
    assert seen["meshes_with_duplicates"] == 15
    v, f = meshes["zeros_19_4"]
    c = O.round_fill(v, f)[2]
    assert (len(v), len(f), c["welded"], c["duplicate_faces"] + c["degenerate_faces"], c["holes3"], c["holes4"]) == (497, 893, 260, 441, 1, 1)
    v, f = meshes["random_18"]
    c = O.round_fill(v, f)[2]
    assert (len(v), len(f), c["welded"], c["duplicate_faces"] + c["degenerate_faces"]) == (1579, 2758, 736, 1208)
    c = O.round_fill(*meshes["noisy_24_9"])[2]
    assert [c[k] for k in O.COUNT_NAMES[2:]] == [0, 0, 0, 0, 8, 0, 0]


def test_clean_is_idempotent_and_leaves_nothing_to_clean():
    for name, (v, f) in fixture_meshes().items():
        vo, fo, info = O.clean(v, f)
        again = O.clean(vo, fo)
        assert same_mesh((vo, fo), again[:2]), name
        keys = O.vertex_keys(vo)
        assert len(np.unique(keys, axis=0)) == len(vo), name                                   # no two vertices share a key
        assert not O.degenerate(vo[fo[:, 0]], vo[fo[:, 1]], vo[fo[:, 2]]).any(), name
        assert len(np.unique(np.sort(fo, axis=1), axis=0)) == len(fo), name                    # no duplicate face
        assert np.array_equal(np.unique(fo), np.arange(len(vo))), name                         # every vertex referenced
        assert info["faces"] == len(fo) and info["vertices"] == len(vo)


def test_clean_meshes_come_back_unchanged_and_small_holes_close():
    meshes = fixture_meshes()
    for name in ("sphere_14_0", "two_20_0"):
        v, f = meshes[name]
        assert same_mesh(O.clean(v, f)[:2], (v, f)), name
    vo, fo, info = O.clean(*meshes["noisy_24_9"])
    assert info["holes3"] == 8 and O.hole_faces(fo, len(vo))[1:] == (0, 0) and len(O.border_edges(fo, len(vo))) == 0


# --------------------------------------------------------------------------------------------------------------- the keyword, on the CPU
def test_clean_keyword_on_a_cpu_device():
    import torch
    from diffudf_amd._lib import DudfError
    from src.render_mc import extract_mesh_MESHUDF
    udf, g = torch.from_numpy(G10["zeros_19_4_udf"]), torch.from_numpy(G10["zeros_19_4_grads"])
    with pytest.raises(DudfError):
        extract_mesh_MESHUDF(udf, g, "cpu", luts=LUTS, clean="device")
    with pytest.raises(ValueError):
        extract_mesh_MESHUDF(udf, g, "cpu", luts=LUTS, clean="trimesh")
    try:
        import trimesh  # noqa: F401
        have_trimesh = True
    except ImportError:
        have_trimesh = False
    v0, f0, m0 = extract_mesh_MESHUDF(udf, g, "cpu", luts=LUTS, clean=False)
    assert (len(m0.vertices), len(m0.faces)) == (497, 893) and v0.dtype == torch.float32 and f0.dtype == torch.int64
    if not have_trimesh:                                                      # the default on a CPU device: the raw arrays, as before
        v1, f1, m1 = extract_mesh_MESHUDF(udf, g, "cpu", smooth_borders=True, luts=LUTS)
        assert np.array_equal(m1.vertices, m0.vertices) and np.array_equal(m1.faces, m0.faces)
        assert torch.equal(v1, v0) and torch.equal(f1, f0)


def test_c_abi_refuses_bad_arguments_on_the_host():
    """Sizes and argument checks are host arithmetic in front of any launch: callable without a GPU."""
    import ctypes
    from diffudf_amd import _lib
    lib = _lib.load()
    need = lib.dudf_mesh_clean_workspace_bytes(1000, 2000)
    # hash tables of at least 2 V, 2 F and 6 F slots (4, 4 and 8 + 4 bytes a slot), the remapped faces, the per-vertex maps
    assert need >= 4 * 2048 + 4 * 4096 + 12 * 16384 + 12 * 2000 + 8 * 1000 and need % 256 == 0
    assert lib.dudf_mesh_clean_workspace_bytes(0, 0) > 0
    assert lib.dudf_mesh_clean_workspace_bytes(1 << 31, 10) == 0 and lib.dudf_mesh_clean_workspace_bytes(10, 1 << 31) == 0
    assert lib.dudf_mesh_clean_workspace_bytes(-1, 10) == 0
    assert lib.dudf_mesh_border_workspace_bytes(1000, 2000) >= 12 * 16384 + 24 * 2000 + 24 * 1000
    assert lib.dudf_mesh_border_workspace_bytes(10, (1 << 32) // 6 + 1) == 0
    P = ctypes.c_void_p
    a = P(256)                                     # a non-null, aligned address that no refused call may touch
    assert lib.dudf_mesh_clean_count(a, 1 << 31, a, 10, 8, 1, a, a, 1 << 40, None) == -4           # DUDF_E_UNSUPPORTED
    assert lib.dudf_mesh_clean_count(a, 10, a, 1 << 31, 8, 1, a, a, 1 << 40, None) == -4
    assert lib.dudf_mesh_clean_count(a, -1, a, 10, 8, 1, a, a, 1 << 40, None) == -1                # DUDF_E_BADCFG
    assert lib.dudf_mesh_clean_count(a, 10, a, 10, 16, 1, a, a, 1 << 40, None) == -1               # digits
    assert lib.dudf_mesh_clean_count(a, 10, a, 10, -1, 1, a, a, 1 << 40, None) == -1
    assert lib.dudf_mesh_clean_count(a, 10, a, 10, 8, 2, a, a, 1 << 40, None) == -1                # fill_holes is 0 or 1
    assert lib.dudf_mesh_clean_count(None, 10, a, 10, 8, 1, a, a, 1 << 40, None) == -1
    assert lib.dudf_mesh_clean_count(a, 10, None, 10, 8, 1, a, a, 1 << 40, None) == -1
    assert lib.dudf_mesh_clean_count(a, 10, a, 10, 8, 1, None, a, 1 << 40, None) == -1
    assert lib.dudf_mesh_clean_count(a, 10, a, 10, 8, 1, a, None, 1 << 40, None) == -2             # DUDF_E_WORKSPACE
    assert lib.dudf_mesh_clean_count(a, 10, a, 10, 8, 1, a, P(264), 1 << 40, None) == -2           # misaligned
    assert lib.dudf_mesh_clean_count(a, 10, a, 10, 8, 1, a, a, lib.dudf_mesh_clean_workspace_bytes(10, 10) - 1, None) == -2
    assert lib.dudf_mesh_clean_emit(a, 10, a, 10, 8, 1, None, a, a, 1 << 40, None) == -1
    assert lib.dudf_mesh_clean_emit(a, 10, a, 10, 8, 1, a, None, a, 1 << 40, None) == -1
    assert lib.dudf_mesh_clean_emit(a, 10, a, 10, 8, 1, a, a, a, 16, None) == -2
    assert lib.dudf_mesh_border_count(10, a, (1 << 32) // 6 + 1, a, a, 1 << 40, None) == -4
    assert lib.dudf_mesh_border_count(10, None, 10, a, a, 1 << 40, None) == -1
    assert lib.dudf_mesh_border_count(10, a, 10, None, a, 1 << 40, None) == -1
    assert lib.dudf_mesh_border_count(10, a, 10, a, a, 16, None) == -2
    assert lib.dudf_mesh_border_edges(10, a, 10, None, a, 1 << 40, None) == -1
    assert lib.dudf_mesh_border_edges(10, a, 10, a, a, 16, None) == -2
    assert lib.dudf_mesh_smooth_borders(a, 10, a, 10, -1, 0.3, a, 1 << 40, None) == -1
    assert lib.dudf_mesh_smooth_borders(None, 10, a, 10, 5, 0.3, a, 1 << 40, None) == -1
    assert lib.dudf_mesh_smooth_borders(a, 10, a, 10, 5, 0.3, a, 16, None) == -2
