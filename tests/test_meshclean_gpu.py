# coding: utf-8
"""GPU: the device mesh clean-up (csrc/dudf_meshclean.hip through the C ABI: `hip_ops.mesh_clean_round`, `mesh_border_edges`,
`mesh_smooth_borders`, `diffudf_amd.meshclean`) against tests/meshclean_oracle.py — vertices, faces and counts bit for bit and in
the same order — on the MeshUDF outputs of the fixtures (tests/test_meshclean_cpu.py asserts that they hold every defect), at the
workgroup and scan boundaries, on inputs that stress the hash tables, and through `extract_mesh_MESHUDF` / `generate_mc`."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshclean_oracle as O  # noqa: E402
import meshtab_cases as M  # noqa: E402
from test_meshclean_cpu import fixture_meshes  # noqa: E402
from test_meshudf import G10, LUTS  # noqa: E402

from diffudf_amd import _lib, hip_ops, meshclean  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def assert_same(got_v, got_f, want_v, want_f, what):
    gv, gf = got_v.cpu().numpy(), got_f.cpu().numpy()
    assert gv.dtype == np.float64 and gf.dtype == np.int64, what
    assert gv.shape == want_v.shape and gf.shape == want_f.shape, (what, gv.shape, want_v.shape, gf.shape, want_f.shape)
    assert gv.tobytes() == want_v.tobytes(), (what, "vertices")
    assert np.array_equal(gf, want_f), (what, "faces", int((gf != want_f).any(axis=1).sum()))


def check_round(v, f, what, fill=True):
    """One device round (with the hole filling) against the oracle's: arrays and all nine counts."""
    wv, wf, wc = O.round_fill(v, f) if fill else O.round(v, f)
    gv, gf, gc = hip_ops.mesh_clean_round(dev(v), dev(f), fill_holes=fill)
    assert gc == wc, (what, gc, wc)
    assert_same(gv, gf, wv, wf, what)
    return wv, wf, wc


def check_clean(v, f, what):
    wv, wf, winfo = O.clean(v, f)
    gv, gf, ginfo = meshclean.clean_mesh(dev(v), dev(f))
    assert ginfo == winfo, (what, ginfo, winfo)
    assert_same(gv, gf, wv, wf, what)
    we = O.border_edges(wf, len(wv))
    ge = meshclean.border_edges(gf, len(wv)).cpu().numpy()
    assert ge.shape == we.shape and np.array_equal(ge, we), (what, "border edges")
    ws = O.smooth(wv, wf)
    gs = meshclean.smooth_borders(gv, gf).cpu().numpy()
    assert gs.tobytes() == ws.tobytes(), (what, "smoothing", float(np.abs(gs - ws).max()))
    return gv, gf, ginfo


def test_fixture_meshes_bit_for_bit():
    meshes = fixture_meshes()
    assert len(meshes) == 47
    for name, (v, f) in meshes.items():
        check_round(v, f, name)
        gv, gf, _ = check_clean(v, f, name)
        if name in ("zeros_19_4", "random_18", "noisy_24_9"):                 # a second run: the same bits
            gv2, gf2, _ = meshclean.clean_mesh(dev(v), dev(f))
            assert torch.equal(gv, gv2) and torch.equal(gf, gf2), name
            s1, s2 = meshclean.smooth_borders(gv, gf), meshclean.smooth_borders(gv, gf)
            assert s1.cpu().numpy().tobytes() == s2.cpu().numpy().tobytes(), name
    # the raw border of a mesh with busy border vertices and faces the round has not yet pruned
    v, f = meshes["random_18"]
    assert np.array_equal(meshclean.border_edges(dev(f), len(v)).cpu().numpy(), O.border_edges(f, len(v)))
    assert meshclean.smooth_borders(dev(v), dev(f), 3, 0.5).cpu().numpy().tobytes() == O.smooth(v, f, 3, 0.5).tobytes()


def coarse_mesh(V, F, seed):
    """V vertices on a coarse lattice (many equal keys, some 4e-9 apart) and F random faces over them."""
    rng = np.random.default_rng(seed)
    side = max(2, int(round(V ** (1 / 3))))
    v = rng.integers(0, side, (V, 3)).astype(np.float64) / side + rng.integers(0, 2, (V, 3)) * 4e-9
    return v, rng.integers(0, V, (F, 3)).astype(np.int64)


@pytest.mark.parametrize("V", [1, 255, 256, 257, 1025])
def test_workgroup_boundaries(V):
    """V and F at 1, 255, 256, 257 (a workgroup takes 256 items) and 1025 (five workgroups, the last with one item).  The scan of
    the workgroup totals gives a thread more than one workgroup beyond 1024 of them: `test_lattice_soup` (1426 workgroups of vertices)."""
    seen = dict(welded=0, degenerate_faces=0, unreferenced=0)
    for F in (1, 255, 256, 257, 1025):
        v, f = coarse_mesh(V, F, 1000 * V + F)
        wv, wf, wc = check_round(v, f, (V, F))
        check_round(v, f, (V, F, "no fill"), fill=False)
        check_clean(v, f, (V, F))
        for k in seen:
            seen[k] += wc[k]
    assert V == 1 or all(n > 0 for n in seen.values()), seen


def test_probe_chain_wraps_round_the_table():
    """`meshtab_cases.wrap_mesh`: three edges whose home is the last of the 32 slots of the edge table, two triples whose home is the
    last of the 8 of the face table.  Four lone triangles: each is a 3-hole of its own."""
    v, f = M.wrap_mesh()
    wc = check_round(v, f, "wrap")[2]
    assert (wc["vertices"], wc["faces"], wc["holes3"], wc["unreferenced"]) == (12, 8, 4, 28)
    assert check_round(v, f, "wrap, no fill", fill=False)[2]["faces"] == 4
    ge = hip_ops.mesh_border_edges(dev(f), len(v)).cpu().numpy()
    assert len(ge) == 12 and np.array_equal(ge, O.border_edges(f, len(v)))


def test_empty_and_all_degenerate(monkeypatch):
    v = np.random.default_rng(0).random((5, 3))
    gv, gf, c = hip_ops.mesh_clean_round(dev(v), torch.zeros(0, 3, dtype=torch.int64, device=DEV), fill_holes=True)
    assert gv.shape == (0, 3) and gf.shape == (0, 3) and c == O.round_fill(v, np.zeros((0, 3), np.int64))[2] and c["unreferenced"] == 5
    gv, gf, info = meshclean.clean_mesh(v, np.zeros((0, 3), np.int64))
    assert gv.shape == (0, 3) and gf.shape == (0, 3) and info["rounds"] == 2
    assert meshclean.border_edges(np.zeros((0, 3), np.int64), 5).shape == (0, 2)
    assert torch.equal(meshclean.smooth_borders(v, np.zeros((0, 3), np.int64)), dev(v))
    calls = []
    real = hip_ops._call
    monkeypatch.setattr(hip_ops, "_call", lambda name, *a, **k: (calls.append(name), real(name, *a, **k))[1])
    f = np.array([[0, 0, 1], [2, 2, 2], [3, 4, 3]])                           # every face degenerate
    gv, gf, c = hip_ops.mesh_clean_round(dev(v), dev(f))
    assert (c["vertices"], c["faces"], c["degenerate_faces"], c["unreferenced"]) == (0, 0, 3, 5)
    assert gv.shape == (0, 3) and gf.shape == (0, 3)
    assert calls == ["dudf_mesh_clean_count"]                                  # the emit launch is not made
    assert c == O.round(v, f)[2]


def lattice_soup(n):
    """The unit squares of n planes z = k of an n^3 lattice, two triangles each, un-indexed: V = 3 F.  Keys k * 10^8 / n in every
    coordinate: a weak hash sends them to a few slots."""
    i, j, k = np.meshgrid(np.arange(n - 1), np.arange(n - 1), np.arange(n), indexing="ij")
    i, j, k = i.reshape(-1), j.reshape(-1), k.reshape(-1)
    p = lambda di, dj: np.stack([i + di, j + dj, k], 1)                       # noqa: E731
    tri = np.concatenate([np.stack([p(0, 0), p(1, 0), p(1, 1)], 1), np.stack([p(0, 0), p(1, 1), p(0, 1)], 1)])
    return tri.reshape(-1, 3).astype(np.float64) / n, np.arange(3 * len(tri), dtype=np.int64).reshape(-1, 3)


def test_lattice_soup():
    v, f = lattice_soup(40)
    assert len(f) == 2 * 39 * 39 * 40 and len(v) == 3 * len(f)
    wv, wf, wc = check_round(v, f, "lattice 40^3")
    assert (wc["vertices"], wc["faces"], wc["welded"]) == (40 ** 3, len(f), len(v) - 40 ** 3)
    ge = meshclean.border_edges(dev(wf), len(wv)).cpu().numpy()
    assert len(ge) == 40 * 4 * 39 and np.array_equal(ge, O.border_edges(wf, len(wv)))


def doubled_mesh(n=5000, F=20000, seed=5):
    """n random vertices, each repeated at index n + i: every key is met twice, far apart, so probe chains grow past one slot."""
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3))
    return np.concatenate([p, p]), rng.integers(0, 2 * n, (F, 3)).astype(np.int64)


def test_every_vertex_duplicated_at_a_far_index():
    v, f = doubled_mesh()
    wv, wf, wc = check_round(v, f, "doubled")
    assert wc["welded"] > 4000 and wc["vertices"] <= 5000
    check_clean(v, f, "doubled")


def test_renumbering_keeps_the_set_of_vertices_and_faces():
    """Exact duplicates and no hole filling (which 4-hole diagonal is taken depends on the numbering): the cleaned mesh is the same
    SET of coordinates and of faces whatever the order of the input."""
    v, f = doubled_mesh(2000, 6000, 9)
    rng = np.random.default_rng(1)
    perm = rng.permutation(len(v))                                             # new index of old vertex i: perm[i]
    v2 = np.empty_like(v); v2[perm] = v
    f2 = perm[f][rng.permutation(len(f))]
    sets = []
    for vv, ff in ((v, f), (v2, f2)):
        gv, gf, _ = meshclean.clean_mesh(vv, ff, fill_holes=False)
        gv, gf = gv.cpu().numpy(), gf.cpu().numpy()
        sets.append((sorted(map(tuple, gv)), sorted(tuple(sorted(map(tuple, gv[t]))) for t in gf)))
    assert sets[0] == sets[1] and len(sets[0][1]) > 5000


def test_invalid_faces_and_argument_errors():
    v, f = coarse_mesh(300, 400, 3)
    v[7] = [np.nan, 0, 0]; v[11, 2] = np.inf
    f[5] = [0, 1, 300]; f[6] = [-1, 2, 3]; f[9] = [2 ** 40, 1, 2]; f[10] = [7, 1, 2]
    wv, wf, wc = check_round(v, f, "invalid")
    assert wc["invalid_faces"] >= 4 + int((f == 11).any(axis=1).sum())
    check_clean(v, f, "invalid")
    assert np.array_equal(meshclean.border_edges(dev(f), 300).cpu().numpy(), O.border_edges(f, 300))
    # a workspace that is too small: an error code, nothing launched
    lib = _lib.load()
    dv, df = dev(v), dev(f)
    need = lib.dudf_mesh_clean_workspace_bytes(300, 400)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    counts = torch.zeros(9, dtype=torch.int64, device=DEV)
    P = lambda t: ctypes.c_void_p(t.data_ptr())                               # noqa: E731
    assert lib.dudf_mesh_clean_count(P(dv), 300, P(df), 400, 8, 1, P(counts), P(ws), need - 1, None) == -2
    assert lib.dudf_mesh_clean_emit(P(dv), 300, P(df), 400, 8, 1, P(dv), P(df), P(ws), need - 1, None) == -2
    nb = lib.dudf_mesh_border_workspace_bytes(300, 400)
    assert lib.dudf_mesh_border_count(300, P(df), 400, P(counts), P(ws), nb - 1, None) == -2
    assert lib.dudf_mesh_smooth_borders(P(dv), 300, P(df), 400, 5, 0.3, P(ws), nb - 1, None) == -2
    assert int(counts.sum()) == 0
    with pytest.raises(_lib.DudfError):
        hip_ops.mesh_clean_round(torch.zeros(3, 3, dtype=torch.float64), torch.zeros(1, 3, dtype=torch.int64))   # CPU tensors


def test_extract_mesh_meshudf_cleans_and_smooths_on_the_device():
    from src.render_mc import extract_mesh_MESHUDF
    udf, g = torch.from_numpy(G10["zeros_19_4_udf"]), torch.from_numpy(G10["zeros_19_4_grads"])
    _, _, raw = extract_mesh_MESHUDF(udf, g, DEV, luts=LUTS, clean=False)
    assert (len(raw.vertices), len(raw.faces)) == (497, 893)
    wv, wf, _ = O.clean(raw.vertices, raw.faces)
    ws = O.smooth(wv, wf)
    try:
        import trimesh  # noqa: F401
        modes = ["device"]                                                    # the default is trimesh's where it is installed
    except ImportError:
        modes = [None, "device"]
    for clean in modes:
        verts, faces, mesh = extract_mesh_MESHUDF(udf, g, DEV, smooth_borders=True, luts=LUTS, clean=clean)
        assert mesh.vertices.tobytes() == ws.tobytes() and np.array_equal(mesh.faces, wf), clean
        assert verts.is_cuda and verts.dtype == torch.float32 and np.array_equal(verts.cpu().numpy(), ws.astype(np.float32))
        assert faces.is_cuda and np.array_equal(faces.cpu().numpy(), wf)
        assert mesh.vertices.shape != raw.vertices.shape and ws.tobytes() != wv.tobytes()
        _, _, plain = extract_mesh_MESHUDF(udf, g, DEV, smooth_borders=False, luts=LUTS, clean=clean)
        assert plain.vertices.tobytes() == wv.tobytes() and np.array_equal(plain.faces, wf)


def test_generate_mc_meshudf_writes_a_clean_mesh(tmp_path):
    from generate_mc import generate_mc
    from src.model import SIREN
    from diffudf_amd import synth
    try:
        import trimesh  # noqa: F401
        pytest.skip("trimesh is installed: generate_mc cleans with it, as the reference")
    except ImportError:
        pass
    m = SIREN(3, 1, [64] * 4, w0=30)
    sd = {}
    for i, (w, b) in enumerate(synth.siren_params([64] * 4, seed=1)):
        sd[f"net.{i}.0.weight"] = torch.from_numpy(w); sd[f"net.{i}.0.bias"] = torch.from_numpy(b)
    m.load_state_dict(sd)
    out = str(tmp_path / "mesh.obj")
    mesh = generate_mc(m, "tanh", 0, 24, out, alpha=100.0, algorithm="meshudf", luts=LUTS)
    v, f = np.asarray(mesh.vertices, np.float64), np.asarray(mesh.faces, np.int64)
    assert len(f) > 1000 and os.path.getsize(out) > 0
    assert len(np.unique(O.vertex_keys(v), axis=0)) == len(v)
    assert not O.degenerate(v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]).any()
    assert np.array_equal(np.unique(f), np.arange(len(v))) and len(np.unique(np.sort(f, axis=1), axis=0)) == len(f)
    lines = open(out).read().splitlines()
    assert sum(l.startswith("v ") for l in lines) == len(v) and sum(l.startswith("f ") for l in lines) == len(f)
