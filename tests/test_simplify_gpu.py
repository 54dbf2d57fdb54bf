# coding: utf-8
"""GPU: the device mesh simplification (csrc/dudf_meshsimplify.hip through the C ABI: `hip_ops.mesh_simplify`,
`diffudf_amd.meshclean.simplify_mesh`) against tests/simplify_oracle.py on the inputs of `simplify_oracle.inputs()` — cell keys, record
counts, faces (order and winding), the counts and, wherever no decision of rule 7 sits within 1e-8 of its threshold, which cells fell
back: EXACTLY; quadrics and xhat within 1e-12 of the cell's largest entry (the order of operations is the oracle's, so equality is
expected: 1e-12 is 4 500 eps); positions within 1e-9 h on those cells (kept components have lam_i > 1e-3 lam_max and the eigensolver's
measured residual is 8.2e-16, tests/test_eigh3_gpu.py: near 1e-12 h, three decades below the bound).  tests/test_simplify_cpu.py caps
the share of the other cells at 2 % for every input.  Then oracle-free properties and the consumers.

Worst figures on an MI355X over all inputs: quadrics 0 and xhat 0 (bit-equal everywhere), positions 4.2e-14 h (CAP sphere 33, grid 12,
w_b = 0); at most 2 of 285 cells below the margin (the planted mesh)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshtab_cases as M  # noqa: E402
import meshtopo_oracle as T  # noqa: E402
import simplify_oracle as S  # noqa: E402
from test_capudf import analytic_fields  # noqa: E402
from test_meshtopo_cpu import same_direction_edges  # noqa: E402

from diffudf_amd import hip_ops, meshclean  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 1e-8
NAMES = list(S.inputs())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(name, w):
    v, f, origin, h, _ = S.inputs()[name]
    return hip_ops.mesh_simplify(dev(v), dev(f), origin, h, boundary_weight=w, want_quadrics=True)


def check(name, w):
    """The device result on an input against the oracle's.  Returns (oracle result, worst quadric, xhat and position figures)."""
    v, f, origin, h, _ = S.inputs()[name]
    return check_mesh(name, w, v, f, origin, h, S.result(name, w))


def check_mesh(name, w, v, f, origin, h, want):
    ov, of, cnt, quad, xhat, keys, records, fell = hip_ops.mesh_simplify(dev(v), dev(f), origin, h, boundary_weight=w, want_quadrics=True)
    assert ov.dtype == torch.float64 and of.dtype == torch.int64 and ov.shape[1:] == (3,) and of.shape[1:] == (3,)
    quad, xhat, keys, records, fell = (t.cpu().numpy() for t in (quad, xhat, keys, records, fell))
    ov, of = ov.cpu().numpy(), of.cpu().numpy()
    wc = want["counts"]
    assert np.array_equal(keys, want["cell_keys"]), (name, w, "cell keys")
    assert np.array_equal(records, want["records"]), (name, w, "records")
    assert np.array_equal(of, want["faces"]), (name, w, "faces")
    sure = want["margin"] >= MARGIN
    assert (~sure).sum() <= 0.02 * max(len(sure), 1), (name, w, "cells below the margin")
    assert {k: cnt[k] for k in S.COUNT_NAMES[:7]} == {k: wc[k] for k in S.COUNT_NAMES[:7]}, (name, w, cnt, wc)
    assert np.array_equal(fell.astype(bool)[sure], want["fell_back"][sure]), (name, w, "fallback cells")
    assert cnt["fallback"] == int(fell.sum()) and cnt["fallback"] - int(fell[~sure].sum()) == wc["fallback"] - int(want["fell_back"][~sure].sum())
    C = len(keys)
    eq = eh = ep = 0.0
    if C:
        scale = np.abs(want["quadrics"]).max(1)
        eq = float((np.abs(quad - want["quadrics"]).max(1) / np.where(scale > 0, scale, 1.0)).max())
        xs = np.abs(want["xhat"]).max(1)
        eh = float((np.abs(xhat - want["xhat"]).max(1) / np.where(xs > 0, xs, 1.0)).max())
    used = want["used"]
    assert ov.shape == want["vertices"].shape and np.isfinite(ov).all(), (name, w)
    if len(ov):
        d = np.abs(ov - want["vertices"]).max(1) / h
        ok = sure[used]
        ep = float(d[ok].max()) if ok.any() else 0.0
        # the cells below the margin: finite (above) and inside their cell, unless the cell's key is saturated
        cells = S.unpack(want["cell_keys"][used][~ok])
        local = (ov[~ok] - origin) / h - cells
        free = ((cells > 0) & (cells < S.CELL_MAX)).all(1)
        assert ((local[free] >= -1e-12) & (local[free] <= 1 + 1e-12)).all(), (name, w, "containment below the margin")
    print(f"{name:28s} w_b = {w}: C = {C}, {int((~sure).sum())} below the margin; quadrics {eq:.2e}, xhat {eh:.2e} (relative to the cell's "
          f"largest entry), positions {ep:.2e} h")
    assert eq <= 1e-12 and eh <= 1e-12, (name, w, eq, eh)
    assert ep <= 1e-9, (name, w, ep)
    return want, (eq, eh, ep)


# ------------------------------------------------------------------------------------------------------------------ against the oracle
def test_empty_one_and_two_faces():
    want, _ = check("F = 0", 1.0)
    assert set(want["counts"].values()) == {0}
    ov, of, cnt = hip_ops.mesh_simplify(dev(np.zeros((5, 3))), dev(np.zeros((0, 3), np.int64)), [0, 0, 0], 1.0)
    assert ov.shape == (0, 3) and of.shape == (0, 3) and set(cnt.values()) == {0}
    for w in (0.0, 1.0):
        assert check("one face", w)[0]["counts"]["faces"] == 1
        assert check("two faces on an edge", w)[0]["counts"]["faces"] == 2


@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_scrambled_strips(n):
    """Across the workgroup size: one cell that holds everything (an empty result, every face collapsed, one run of n records), and a
    lattice below the vertex spacing (the identity up to the order of the vertices)."""
    want, _ = check(f"strip {n}, one cell", 1.0)
    c = want["counts"]
    assert (c["vertices"], c["faces"], c["cells"], c["collapsed"]) == (0, 0, 1, n) and want["records"].tolist() == [n]
    want, _ = check(f"strip {n}, fine", 1.0)
    c = want["counts"]
    assert (c["vertices"], c["faces"], c["collapsed"], c["duplicate"]) == (n + 2, n, 0, 0)
    v, f, origin, h, _ = S.inputs()[f"strip {n}, fine"]
    ov, of, _ = hip_ops.mesh_simplify(dev(v), dev(f), origin, h)
    assert np.abs(ov.cpu().numpy()[of.cpu().numpy()] - v[f]).max() <= 1e-9 * h        # the same triangles, corner by corner


@pytest.mark.parametrize("grid", [8, 7])
@pytest.mark.parametrize("w", [0.0, 1.0])
def test_grid_plane(grid, w):
    want, _ = check(f"grid plane, grid {grid}", w)
    assert want["counts"]["faces"] == 2 * grid * grid and want["counts"]["border_edges"] == 256


def test_probe_chain_wraps_round_the_table():
    """`meshtab_cases.wrap_mesh`: three edges whose home is the last of the 32 slots.  Every vertex has its own cell: the identity up to
    the order of the vertices, 12 border edges."""
    v, f = M.wrap_mesh()
    for w in (0.0, 1.0):
        c = check_mesh("wrap", w, v, f, np.zeros(3), M.WRAP_H, S.simplify(v, f, np.zeros(3), M.WRAP_H, w))[0]["counts"]
        assert (c["vertices"], c["faces"], c["cells"], c["border_edges"]) == (12, 4, 12, 12)


def test_a_thousand_tetrahedra():
    want, _ = check("tetrahedra, coarse", 1.0)
    assert want["counts"]["collapsed"] == 4000 and want["counts"]["cells"] == 1000 and want["counts"]["faces"] == 0
    want, _ = check("tetrahedra, fine", 1.0)
    assert want["counts"]["faces"] == 4000 and want["counts"]["border_edges"] == 0


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("CAP ")])
@pytest.mark.parametrize("w", [0.0, 1.0])
def test_welded_cap_udf_soups(name, w):
    want, _ = check(name, w)
    assert 0 < want["counts"]["faces"] < len(S.inputs()[name][1]) and want["counts"]["border_edges"] > 0


@pytest.mark.parametrize("w", [0.0, 1.0])
def test_planted_defects(w):
    want, _ = check("planted", w)
    _, _, facts = S.planted()
    c = want["counts"]
    assert c["invalid"] == facts["invalid"] and c["duplicate"] == facts["duplicate"] and c["collapsed"] > facts["repeated"]
    assert facts["corner_key"] in want["cell_keys"].tolist() and all(k in want["cell_keys"].tolist() for k in facts["saturated_keys"])


# ------------------------------------------------------------------------------------------------------------------ without the oracle
def test_properties():
    v, f = T.cap_welded("sheet", 65)
    h = S.extent(v) / 23
    origin = S.centred_origin(v, h)
    ov, of, cnt, quad, xhat, keys, records, fell = hip_ops.mesh_simplify(dev(v), dev(f), origin, h, want_quadrics=True)
    p, g = ov.cpu().numpy(), of.cpu().numpy()
    assert len(g) == cnt["faces"] > 100 and len(p) == cnt["vertices"]
    # the used cells, recounted from the input alone: the cells of the faces whose corners lie in three cells, ascending; vertex i lies
    # in the i-th of them to within one part in 10^12 of h
    ck = S.pack(S.vertex_cells(v[f], origin, 1.0 / h))
    three = (ck[:, 0] != ck[:, 1]) & (ck[:, 1] != ck[:, 2]) & (ck[:, 2] != ck[:, 0])
    used = np.unique(ck[three])
    assert len(used) == len(p) and set(used.tolist()) <= set(keys.cpu().numpy().tolist())
    local = (p - origin) / h - S.unpack(used)
    assert ((local >= -1e-12) & (local <= 1 + 1e-12)).all()
    # no face has a repeated index, no two faces share a vertex set, every vertex is used
    assert (g[:, 0] != g[:, 1]).all() and (g[:, 1] != g[:, 2]).all() and (g[:, 2] != g[:, 0]).all()
    assert len(set(map(tuple, np.sort(g, 1).tolist()))) == len(g)
    assert np.array_equal(np.unique(g), np.arange(len(p)))
    # two runs are equal bit for bit
    again = hip_ops.mesh_simplify(dev(v), dev(f), origin, h, want_quadrics=True)
    assert all(torch.equal(a, b) for a, b in zip((ov, of, quad, xhat, keys, records, fell), again[:2] + again[3:])) and again[2] == cnt
    # the count-only form agrees and places nothing
    only = hip_ops.mesh_simplify_count(dev(v), dev(f), origin, h)
    assert only["fallback"] == -1 and all(only[k] == cnt[k] for k in S.COUNT_NAMES[:7])
    with pytest.raises(Exception):
        hip_ops.mesh_simplify(torch.from_numpy(v), torch.from_numpy(f), origin, h)      # CPU tensors: no fallback


def test_simplify_mesh_keywords():
    v, f = T.cap_welded("sheet", 65)
    t = 400
    ov, of, info = meshclean.simplify_mesh(dev(v), dev(f), target_faces=t, orient=True)
    print(f"target_faces = {t}: grid {info['grid']}, {info['faces']} faces of {len(f)}, {info['count_calls']} count calls")
    assert 0 < of.shape[0] <= t and info["count_calls"] <= 21 and info["grid"] >= 1 and info["faces"] == of.shape[0]
    topo = meshclean.face_topology(of, ov.shape[0], ov)
    assert topo["inconsistent_edges"] == 0 and same_direction_edges(of.cpu().numpy(), ov.shape[0]) == 0
    # the chosen lattice is what grid= gives, and its origin is the bounding-box minimum
    gv, gf, ginfo = meshclean.simplify_mesh(dev(v), dev(f), grid=info["grid"], orient=True)
    assert torch.equal(gv, ov) and torch.equal(gf, of) and ginfo["origin"] == v.min(0).tolist() and ginfo["count_calls"] == 0
    cv, cf, _ = meshclean.simplify_mesh(dev(v), dev(f), cell=ginfo["cell"])
    assert torch.equal(cv, ov) and cf.shape == of.shape
    # a target nothing meets ends at the coarsest lattice
    _, nf, ninfo = meshclean.simplify_mesh(dev(v), dev(f), target_faces=-1)
    assert ninfo["grid"] == 1 and nf.shape[0] == 0 and ninfo["count_calls"] <= 21


# ------------------------------------------------------------------------------------------------------------------------- consumers
def test_extract_mesh_cap_finish_simplify():
    from src.render_mc import SparseFields, extract_mesh_CAP, extract_mesh_CAP_sparse
    n = 33
    ndf, vec = analytic_fields(n, "sheet")
    d, g = dev(ndf), dev(vec)
    mesh = extract_mesh_CAP(d, g, n, finish={"simplify": {"grid": 12}})
    sv, sf = hip_ops.capudf_extract(d, g, 0.008)
    cv, cf, _ = meshclean.clean_mesh(sv, sf, fill_holes=False)
    cv, cf, _ = meshclean.remove_small_components(cv, cf)
    wv, wf, info = meshclean.simplify_mesh(cv, cf, grid=12, orient=True)
    assert 0 < info["faces"] < cf.shape[0]
    assert np.asarray(mesh.vertices).tobytes() == wv.cpu().numpy().tobytes() and np.array_equal(np.asarray(mesh.faces), wf.cpu().numpy())
    # without the key: what finish= gave before
    plain = extract_mesh_CAP(d, g, n, finish="mesh")
    assert len(plain.faces) == cf.shape[0] > len(mesh.faces)
    sp = extract_mesh_CAP_sparse(SparseFields.from_dense(d, g), finish={"simplify": {"grid": 12}, "min_faces": 1})
    assert 0 < len(sp.faces) < cf.shape[0] and same_direction_edges(np.asarray(sp.faces), len(sp.vertices)) == 0
    with pytest.raises(ValueError):
        extract_mesh_CAP(d, g, n, finish={"simplify": {"faces": 3}})


def test_generate_mc_keys(tmp_path):
    import generate_mc
    from test_meshtopo_gpu import read_obj
    from test_sparse_mc_gpu import PLANE_FIELDS, plane_model
    N = 33
    mode, alpha = PLANE_FIELDS["fold"]
    model = plane_model([32] * 2, "fold")
    p = lambda name: str(tmp_path / name)  # noqa: E731
    # the keys absent: the call without them, byte for byte
    generate_mc.generate_mc(model, mode, 0, N, p("a.obj"), alpha, algorithm="cap", cap_finish="mesh")
    full = generate_mc.generate_mc(model, mode, 0, N, p("b.obj"), alpha, algorithm="cap", cap_finish="mesh", simplify_target_faces=None,
                                   simplify_grid=None, simplify_boundary_weight=None)
    assert open(p("a.obj"), "rb").read() == open(p("b.obj"), "rb").read() and len(full.faces) > 100
    t = len(full.faces) // 4
    small = generate_mc.generate_mc(model, mode, 0, N, p("small.obj"), alpha, algorithm="cap", simplify_target_faces=t)
    v, f = read_obj(p("small.obj"))
    assert 0 < len(f) <= t and np.array_equal(f, np.asarray(small.faces)) and same_direction_edges(f, len(v)) == 0
    wv, wf, _ = meshclean.simplify_mesh(dev(np.asarray(full.vertices)), dev(np.asarray(full.faces)), target_faces=t, orient=True)
    assert np.array_equal(wf.cpu().numpy(), f) and wv.cpu().numpy().tobytes() == np.asarray(small.vertices).tobytes()
    grid = generate_mc.generate_mc(model, mode, 0, N, p("grid.obj"), alpha, algorithm="cap", simplify_grid=6, simplify_boundary_weight=0.0)
    gv, gf, _ = meshclean.simplify_mesh(dev(np.asarray(full.vertices)), dev(np.asarray(full.faces)), grid=6, boundary_weight=0.0, orient=True)
    assert np.array_equal(gf.cpu().numpy(), np.asarray(grid.faces)) and 0 < len(grid.faces) < len(full.faces)
    sparse = generate_mc.generate_mc(model, mode, 0, N, p("sparse.obj"), alpha, algorithm="cap", sparse=True, simplify_grid=6)
    assert 0 < len(sparse.faces) < len(full.faces)
