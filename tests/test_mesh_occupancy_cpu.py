# coding: utf-8
"""CPU: the occupancy / mesh-march entry points are declared, exported and bound; their host-side argument checks; the numpy
restatement of the crossing rule on the lattice cube; the reference-named GT renderer still raises."""
import ctypes
import os
import re

import numpy as np
import pytest

import mesh_occupancy_oracle as OO
from diffudf_amd import _lib, hip_ops, metrics, render_st

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dudf_mesh_occupancy", "dudf_mesh_trace_rays")
OK, E_CFG, E_WS = 0, -1, -2


def test_header_declares_and_library_exports_the_new_calls():
    src = open(os.path.join(REPO, "include", "dudf_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert lib.dudf_abi_version() == _lib.ABI_VERSION == 8                       # no existing signature changed
    for name in ("mesh_occupancy", "mesh_trace_rays"):
        assert callable(getattr(hip_ops, name))
    for name in ("occupancy", "signed_distance", "trace_rays"):
        assert callable(getattr(metrics.MeshIndex, name))
    assert callable(render_st.create_projectional_image_mesh)
    import generate_st
    assert generate_st.create_projectional_image_mesh is render_st.create_projectional_image_mesh


def test_host_side_argument_checks():
    """Every return here happens before the first HIP call: the pointers are a host address that is never dereferenced."""
    lib = _lib.load()
    arena = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.addressof(arena) + 255) // 256 * 256
    P, n = ctypes.c_void_p(base), 8
    nb = int(lib.dudf_mesh_index_bytes(n))
    occ = lambda index, nbytes, q=n: lib.dudf_mesh_occupancy(P, n, index, nbytes, P, q, P, P, None)                   # noqa: E731
    assert occ(ctypes.c_void_p(base + 8), nb) == E_WS and occ(P, nb - 1) == E_WS
    assert occ(None, 0, 0) == OK and occ(P, nb, -1) == E_CFG
    assert lib.dudf_mesh_occupancy(None, n, P, nb, P, n, P, P, None) == E_CFG
    assert lib.dudf_mesh_occupancy(P, 0, None, 0, P, n, P, P, None) == E_CFG
    trace = lambda index, nbytes, m=n, it=30, t0=P: lib.dudf_mesh_trace_rays(P, n, index, nbytes, P, t0, P, P, m, 0.001, it, 1.3, None)   # noqa: E731
    assert trace(ctypes.c_void_p(base + 8), nb) == E_WS and trace(P, nb - 1) == E_WS
    assert trace(None, 0, 0) == OK and trace(P, nb, -1) == E_CFG
    assert trace(P, nb, n, -1) == E_CFG and trace(P, nb, n, 30, None) == E_CFG


def test_oracle_on_the_lattice_cube():
    """The numpy restatement on its own: 12 triangles, 729 lattice points whose (y, z) fall on edges, the face diagonals and the
    vertices with exact edge functions; the footprint is half-open as the tie rule says, and no crossing is counted twice."""
    v, f = OO.cube()
    tri = OO.soup(v, f)
    p = OO.lattice(9, 0.25)
    count, margin = OO.crossings(p, tri)
    assert set(np.unique(count)) == {0, 1, 2}
    assert (margin == 0).sum() > 100
    inside = (count & 1).astype(bool)
    assert inside.sum() == 64 and np.array_equal(inside, OO.cube_inside(p))
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    foot = (y > -0.5) & (y <= 0.5) & (z >= -0.5) & (z < 0.5)
    assert np.array_equal(count, np.where(foot, (x < 0.5).astype(int) + (x < -0.5).astype(int), 0))
    # the answer does not depend on how the faces are split or listed: the other diagonal, reversed order, rotated vertices
    f2 = np.concatenate([np.stack([f[0::2, 0], f[0::2, 1], f[1::2, 2]], axis=1), np.stack([f[0::2, 1], f[0::2, 2], f[1::2, 2]], axis=1)])
    for faces in (f[::-1], np.roll(f, 1, axis=1), f2):
        assert np.array_equal(OO.crossings(p, OO.soup(v, faces))[0], count)
    q = p.copy(); q[3, 1] = np.nan
    assert OO.crossings(q, tri)[0][3] == -1


def test_gt_renderer_still_raises_and_names_the_new_one():
    from src.render_st import create_projectional_image_gt
    with pytest.raises(_lib.DudfError, match="open3d") as e:
        create_projectional_image_gt("mesh.obj", 4, 4, None, None, None, None, False)
    assert "create_projectional_image_mesh" in str(e.value)
    with pytest.raises(_lib.DudfError, match="GPU"):
        render_st.create_projectional_image_mesh("mesh.obj", 4, 4, None, None, None, [0, 0, 1], device="cpu")
