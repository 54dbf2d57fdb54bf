# coding: utf-8
"""GPU: the device mesh topology (csrc/dudf_meshtopo.hip through the C ABI: `hip_ops.mesh_topology`, `mesh_submesh`,
`diffudf_amd.meshclean.face_topology` / `orient_faces` / `remove_small_components`) against tests/meshtopo_oracle.py — oriented faces,
components, flips, per-component face counts and integer areas and all eight counts EXACTLY — on chains across the workgroup and
pointer-doubling boundaries, planted defects, lattice keys and the welded CAP-UDF soups (tests/test_meshtopo_cpu.py asserts that one
manifold edge in six of those is inconsistent), oracle-free properties, the component filter at its integer thresholds, and the
`finish=` keyword of the CAP-UDF extractors and `generate_mc`."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshtab_cases as M  # noqa: E402
import meshtopo_oracle as T  # noqa: E402
from test_capudf import analytic_fields  # noqa: E402
from test_meshtopo_cpu import same_direction_edges  # noqa: E402

from diffudf_amd import hip_ops, meshclean  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check(v, f, what, n_vertices=None):
    """The device result against the oracle's: every array and all eight counts.  Returns the oracle's."""
    V = len(v) if n_vertices is None else n_vertices
    want = T.topology(f, V, v)
    of, comp, flip, nfaces, area_q, cnt = hip_ops.mesh_topology(dev(f), V, None if v is None else dev(v))
    assert cnt == {k: want[k] for k in T.COUNT_NAMES}, (what, cnt, {k: want[k] for k in T.COUNT_NAMES})
    assert of.dtype == torch.int64 and comp.dtype == torch.int64 and flip.dtype == torch.uint8
    assert np.array_equal(flip.cpu().numpy(), want["flip"]), (what, "flip")
    assert np.array_equal(comp.cpu().numpy(), want["component"]), (what, "component")
    assert np.array_equal(of.cpu().numpy(), want["faces"]), (what, "faces")
    assert np.array_equal(nfaces.cpu().numpy(), want["component_faces"]), (what, "component_faces")
    assert np.array_equal(area_q.cpu().numpy().view(np.uint64), want["component_area_q"]), (what, "component_area_q")
    got = meshclean.face_topology(dev(f), V, None if v is None else dev(v))
    assert np.array_equal(got["labels"], want["labels"]) and np.array_equal(got["n_faces"], want["n_faces"]), what
    if v is None:
        assert got["area"] is None and got["area_q"] is None
    else:
        assert got["area_q"].dtype == np.uint64 and np.array_equal(got["area_q"], want["area_q"]), what
        assert got["area"].tobytes() == want["area"].tobytes(), what
    assert torch.equal(got["faces"], of) and torch.equal(got["component"], comp) and torch.equal(got["flip"], flip)
    assert all(got[k] == want[k] for k in T.COUNT_NAMES)
    return want


def combine(*meshes):
    vs, fs, base = [], [], 0
    for v, f in meshes:
        vs.append(v); fs.append(f + base); base += len(v)
    return np.concatenate(vs), np.concatenate(fs)


# ------------------------------------------------------------------------------------------------------------------ against the oracle
def test_empty_one_and_two_faces():
    r = check(np.zeros((0, 3)), np.zeros((0, 3), np.int64), "F = 0")
    assert r["components"] == 0
    of, comp, flip, nfaces, area_q, cnt = hip_ops.mesh_topology(dev(np.zeros((0, 3), np.int64)), 5)
    assert of.shape == (0, 3) and comp.shape == (0,) and set(cnt.values()) == {0}
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], np.float64)
    assert check(v, np.array([[0, 1, 2]]), "F = 1")["border_edges"] == 3
    assert check(v, np.array([[0, 1, 2], [1, 0, 3]]), "two, opposite")["flipped_faces"] == 0
    assert check(v, np.array([[0, 1, 2], [0, 1, 3]]), "two, same")["flipped_faces"] == 1
    assert check(None, np.array([[0, 1, 2], [0, 1, 3]]), "no vertices", n_vertices=4)["flipped_faces"] == 1


@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_scrambled_strips(n):
    """One chain of n - 1 links: the longest path the hooks can build, across the workgroup size and the doubling steps."""
    v, f = T.strip(n)
    r = check(v, T.scramble(f, n), f"strip {n}")
    assert r["components"] == 1 and r["forest_edges"] == n - 1 and r["inconsistent_edges"] == 0 and 0 < r["flipped_faces"] < n
    check(v, f, f"strip {n}, in order")                  # keys ascend along the chain: every round hooks a long run


def test_planted_defects():
    v, f = T.mobius(12)
    assert check(v, f, "moebius")["inconsistent_edges"] >= 1
    assert check(v, T.scramble(f, 3), "moebius, scrambled")["inconsistent_edges"] >= 1
    v, f = T.fin()
    r = check(v, f, "fin")
    assert (r["components"], r["nonmanifold_edges"]) == (3, 1)
    check(v[:3], np.array([[0, 1, 2], [0, 1, 2]]), "duplicate")
    v, f = T.strip(300)
    g = T.scramble(f, 11)
    g[0] = [0, 0, 1]; g[-1] = [5, 6, len(v)]             # ignored faces at the first and the last index
    r = check(v, g, "ignored at the ends")
    assert r["ignored_faces"] == 2 and r["component"][0] == 0 and r["component"][-1] == len(g) - 1
    g[7] = [-1, 2, 3]; g[150] = [3, 2 ** 40, 4]
    assert check(v, g, "ignored, far indices")["ignored_faces"] == 4
    nanv = v.copy(); nanv[9] = np.nan; nanv[20] *= 1e200   # a NaN and an overflowing face normal weigh nothing / saturate
    check(nanv, T.scramble(f, 12), "non-finite areas")


def test_a_thousand_tetrahedra():
    v, f = T.tetrahedra(1000)
    r = check(v, T.scramble(f, 21), "1000 tetrahedra")
    assert r["components"] == 1000 and r["forest_edges"] == 3000 and r["n_faces"].tolist() == [4] * 1000
    assert len(set(r["area_q"].tolist())) > 900


def test_grid_plane_lattice_keys():
    v, f = T.grid_plane(64, 64)
    r = check(v, T.scramble(f, 31), "grid 64 x 64")
    assert len(f) == 8192 and r["components"] == 1 and r["inconsistent_edges"] == 0 and r["border_edges"] == 256


def test_probe_chain_wraps_round_the_table():
    """`meshtab_cases.wrap_mesh`: three edges whose home is the last of the 32 slots."""
    v, f = M.wrap_mesh()
    r = check(v, f, "wrap")
    assert (r["components"], r["border_edges"], r["ignored_faces"]) == (4, 12, 0)


def test_the_three_edge_tables_agree():
    """The clean-up's, the topology's and the simplification's edge table on one mesh of valid faces without repeated indices: the
    edges with one use, counted in numpy; the topology's edges with three or more.  Without and with a third face on one edge."""
    for extra_face in (False, True):
        v, f = M.holed_grid(extra_face)
        uses = M.edge_use_counts(f)
        border, fins = int((uses == 1).sum()), int((uses >= 3).sum())
        assert border > 64 and fins == int(extra_face)
        assert len(hip_ops.mesh_border_edges(dev(f), len(v))) == border
        cnt = hip_ops.mesh_topology(dev(f), len(v), dev(v))[5]
        assert (cnt["border_edges"], cnt["nonmanifold_edges"]) == (border, fins), cnt
        assert hip_ops.mesh_simplify_count(dev(v), dev(f), [0.0, 0.0, -0.5], 1.0 / 64)["border_edges"] == border


@pytest.mark.parametrize("kind,n", [("sheet", 33), ("sphere", 33), ("sheet", 65)])
def test_welded_cap_udf_soups(kind, n):
    v, f = T.cap_welded(kind, n)
    r = check(v, f, f"CAP {kind} {n}")
    assert r["inconsistent_edges"] == 0 and r["flipped_faces"] > 100


# ------------------------------------------------------------------------------------------------------------------ without the oracle
def test_properties():
    v, f = combine(T.grid_plane(20, 13), T.tetrahedra(30), T.strip(77))
    g = T.scramble(f, 41)
    V = len(v)
    a = meshclean.face_topology(dev(g), V, dev(v))
    of = a["faces"].cpu().numpy()
    assert a["inconsistent_edges"] == 0 and same_direction_edges(of, V) == 0 and same_direction_edges(g, V) > 0
    again = meshclean.face_topology(a["faces"], V, dev(v))                      # orienting an oriented mesh flips nothing
    assert again["flipped_faces"] == 0 and torch.equal(again["faces"], a["faces"])
    assert torch.equal(meshclean.orient_faces(dev(v), dev(g)), a["faces"])
    # a permutation of the faces gives the same partition (labels are positions, so compare the sets of faces)
    perm = np.random.default_rng(5).permutation(len(g))
    b = meshclean.face_topology(dev(g[perm]), V, dev(v))
    part = lambda comp, order: sorted(sorted(order[np.nonzero(comp == c)[0]].tolist()) for c in np.unique(comp))  # noqa: E731
    assert part(a["component"].cpu().numpy(), np.arange(len(g))) == part(b["component"].cpu().numpy(), perm)
    assert sorted(a["area_q"].tolist()) == sorted(b["area_q"].tolist()) and b["inconsistent_edges"] == 0
    # two runs give the same bytes
    x = hip_ops.mesh_topology(dev(g), V, dev(v))
    y = hip_ops.mesh_topology(dev(g), V, dev(v))
    assert all(torch.equal(p, q) for p, q in zip(x[:5], y[:5])) and x[5] == y[5]
    with pytest.raises(Exception):
        hip_ops.mesh_topology(torch.from_numpy(g), V)                            # a CPU tensor: no fallback


# ---------------------------------------------------------------------------------------------------------------- filter and submesh
def filtered(v, f, **kw):
    wv, wf, wc = T.remove_small_components(v, f, **kw)
    gv, gf, info = meshclean.remove_small_components(dev(v), dev(f), **kw)
    assert gv.dtype == torch.float64 and gf.dtype == torch.int64
    assert (gv.shape[0], gf.shape[0]) == wc, (kw, gv.shape, gf.shape, wc)
    assert gv.cpu().numpy().tobytes() == wv.tobytes() and np.array_equal(gf.cpu().numpy(), wf), kw
    assert info["faces_removed"] == len(f) - wc[1]
    return wc, info


def test_filter_at_the_integer_thresholds():
    a, b, c = T.strip(4), T.strip(5), T.strip(12)        # unit right triangles: q = 2^30 a face, areas 2, 2.5 and 6
    v, f = combine(a, b, c)
    g = T.scramble(f, 51)
    assert filtered(v, g, min_faces=5)[0] == (7 + 14, 17)                        # exactly min_faces stays, min_faces - 1 goes
    assert filtered(v, g, min_faces=4)[0] == (len(v), 21)
    assert filtered(v, g, min_faces=6)[0] == (14, 12)
    assert filtered(v, g, min_area=2.0)[0][1] == 21 and filtered(v, g, min_area=2.0 + 2.0 ** -31)[0][1] == 17
    v2, f2 = combine(a, c)                               # sum 2^34: a quarter is exactly the smaller component
    g2 = T.scramble(f2, 52)
    assert filtered(v2, g2, min_area_ratio=0.25)[0][1] == 16 and filtered(v2, g2, min_area_ratio=0.25 + 2.0 ** -33)[0][1] == 12
    v3, f3 = combine(b, a, b)                            # two components tie in (area, faces): the smaller label stays
    wc, info = filtered(v3, f3, keep_largest=1)
    assert wc == (7, 5) and info["components_kept"] == 1 and info["components_removed"] == 2
    gv, gf, _ = meshclean.remove_small_components(dev(v3), dev(f3), keep_largest=1)
    assert gv.cpu().numpy().tobytes() == b[0].tobytes()                          # the FIRST strip of five
    assert filtered(v3, T.scramble(f3, 53), keep_largest=2)[0] == (14, 10)
    assert filtered(v3, f3, min_faces=5, keep_largest=3)[0] == (14, 10)
    assert filtered(v3, f3, min_faces=100)[0] == (0, 0)


def test_submesh_against_the_oracle():
    v, f = T.cap_welded("sheet", 33)
    rng = np.random.default_rng(61)
    for keep in (rng.random(len(f)) < 0.5, np.ones(len(f), bool), np.zeros(len(f), bool), np.arange(len(f)) == len(f) - 1):
        wv, wf, wc = T.submesh(v, f, keep)
        gv, gf = hip_ops.mesh_submesh(dev(v), dev(f), dev(keep))
        assert (gv.shape[0], gf.shape[0]) == wc and gv.shape[1:] == (3,) and gf.shape[1:] == (3,)
        assert gv.cpu().numpy().tobytes() == wv.tobytes() and np.array_equal(gf.cpu().numpy(), wf)
    bad = f.copy(); bad[3, 1] = len(v); bad[10, 0] = -1  # kept faces that cannot be re-indexed go
    wv, wf, wc = T.submesh(v, bad, np.ones(len(f), bool))
    gv, gf = hip_ops.mesh_submesh(dev(v), dev(bad), dev(np.ones(len(f), np.uint8)))
    assert wc[1] == len(f) - 2 and gv.cpu().numpy().tobytes() == wv.tobytes() and np.array_equal(gf.cpu().numpy(), wf)


# ------------------------------------------------------------------------------------------------------------------------- end to end
def tri_set(v, f):
    """The triangles as a sorted (F, 9) array, each triangle's three vertices in lexicographic order: winding and order removed."""
    p = np.asarray(v, np.float64)[np.asarray(f, np.int64)]
    p = np.stack([t[np.lexsort(t.T[::-1])] for t in p]).reshape(len(p), 9) if len(p) else p.reshape(0, 9)
    return p[np.lexsort(p.T[::-1])]


def test_extract_mesh_cap_finish():
    from src.render_mc import SparseFields, extract_mesh_CAP, extract_mesh_CAP_sparse
    n = 33
    ndf, vec = analytic_fields(n, "sheet")
    d, g = dev(ndf), dev(vec)
    # finish=None: today's soup
    sv, sf = hip_ops.capudf_extract(d, g, 0.008)
    soup = extract_mesh_CAP(d, g, n)
    assert np.array_equal(np.asarray(soup.vertices), sv.cpu().numpy()) and np.array_equal(np.asarray(soup.faces), sf.cpu().numpy())
    # finish="mesh": the oracle chain, bit for bit
    wv, wf = T.cap_welded("sheet", n)
    assert len(soup.vertices) > len(wv) and len(soup.faces) >= len(wf)      # per-cell vertices: nothing welded
    want = T.topology(wf, len(wv), wv)
    mesh = extract_mesh_CAP(d, g, n, finish="mesh")
    gv, gf = np.asarray(mesh.vertices), np.asarray(mesh.faces)
    print(f"finish='mesh' sheet {n}: {gv.shape} / {wv.shape} vertices, {gf.shape} / {wf.shape} faces, max |dv| "
          f"{np.abs(gv - wv).max() if gv.shape == wv.shape else float('nan'):.3e}")
    assert type(mesh) is type(soup) and gv.shape == wv.shape and gf.shape == wf.shape
    assert np.array_equal(gf, want["faces"]) and gv.tobytes() == wv.tobytes()
    assert same_direction_edges(gf, len(gv)) == 0 and same_direction_edges(wf, len(wv)) == 141
    # a dict: the same, then the filter
    small = extract_mesh_CAP(d, g, n, finish={"min_faces": 97})
    ov, of_, oc = T.remove_small_components(wv, wf, min_faces=97)
    assert oc[1] == 180 + 180 + 97 and np.asarray(small.vertices).tobytes() == ov.tobytes() and np.array_equal(np.asarray(small.faces), of_)
    one = extract_mesh_CAP(d, g, n, finish={"keep_largest": 1, "min_area_ratio": 0.01})
    assert len(one.faces) == 180
    with pytest.raises(ValueError):
        extract_mesh_CAP(d, g, n, finish="weld")
    # the sparse path: the same triangles
    sp = extract_mesh_CAP_sparse(SparseFields.from_dense(d, g), finish="mesh")
    a, b = tri_set(sp.vertices, sp.faces), tri_set(gv, gf)
    print(f"sparse / dense finish='mesh': {a.shape} / {b.shape} triangles, max |d| {np.abs(a - b).max() if a.shape == b.shape else float('nan'):.3e}")
    assert len(sp.faces) == len(gf) and np.array_equal(tri_set(sp.vertices, sp.faces), tri_set(gv, gf))
    assert same_direction_edges(np.asarray(sp.faces), len(sp.vertices)) == 0
    plain = extract_mesh_CAP_sparse(SparseFields.from_dense(d, g))
    assert len(plain.vertices) == len(soup.vertices) and len(plain.faces) == len(soup.faces)


def read_obj(path):
    rows = [ln.split() for ln in open(path)]
    return (np.array([[float(x) for x in r[1:]] for r in rows if r[0] == "v"]).reshape(-1, 3),
            np.array([[int(x) for x in r[1:]] for r in rows if r[0] == "f"], np.int64).reshape(-1, 3) - 1)


def test_generate_mc_filter_reaches_the_meshudf_mesh(tmp_path):
    """The device-cleaned MeshUDF mesh of 'meshudf' loses the components the keys reject; without the keys it is what it was."""
    try:
        import trimesh  # noqa: F401
        have_trimesh = True
    except ImportError:
        have_trimesh = False
    from generate_mc import generate_mc
    from src.model import SIREN
    from diffudf_amd import synth
    from test_meshudf import LUTS
    m = SIREN(3, 1, [64] * 4, w0=30)
    sd = {}
    for i, (w, b) in enumerate(synth.siren_params([64] * 4, seed=1)):
        sd[f"net.{i}.0.weight"] = torch.from_numpy(w); sd[f"net.{i}.0.bias"] = torch.from_numpy(b)
    m.load_state_dict(sd)
    full = generate_mc(m, "tanh", 0, 24, str(tmp_path / "full.obj"), alpha=100.0, algorithm="meshudf", luts=LUTS)
    v, f = np.asarray(full.vertices, np.float64), np.asarray(full.faces, np.int64)
    t = T.topology(f, len(v), v)
    print(f"MeshUDF mesh: {len(f)} faces in {t['components']} components, largest {int(t['n_faces'].max())}")
    assert t["components"] > 1                           # a random network's level set at 24^3 comes in pieces
    k = int(np.sort(t["n_faces"])[-1])
    kept = generate_mc(m, "tanh", 0, 24, str(tmp_path / "kept.obj"), alpha=100.0, algorithm="meshudf", luts=LUTS, min_component_faces=k)
    ov, of_, oc = T.remove_small_components(v, f, min_faces=k)
    assert 0 < oc[1] < len(f) and np.array_equal(np.asarray(kept.faces), of_)
    if not have_trimesh:
        assert np.asarray(kept.vertices).tobytes() == ov.tobytes()
    gv, gf = read_obj(str(tmp_path / "kept.obj"))
    assert np.array_equal(gf, of_) and len(gv) == oc[0]


def test_generate_mc_keys(tmp_path):
    import generate_mc
    from src.render_mc import extract_fields, extract_mesh_CAP
    from test_sparse_mc_gpu import PLANE_FIELDS, plane_model
    N = 33
    mode, alpha = PLANE_FIELDS["fold"]
    model = plane_model([32] * 2, "fold")
    d = torch.device(DEV)
    p = lambda name: str(tmp_path / name)  # noqa: E731
    # without the keys: the file the extraction functions write, byte for byte
    generate_mc.generate_mc(model, mode, 0, N, p("plain.obj"), alpha, algorithm="cap")
    soup = extract_mesh_CAP(*extract_fields(model, torch.Tensor([[]]).to(d), N, mode, d, alpha), N)
    soup.export(p("want.obj"))
    assert open(p("plain.obj"), "rb").read() == open(p("want.obj"), "rb").read() and len(soup.faces) > 0
    # "cap_finish": "mesh"
    mesh = generate_mc.generate_mc(model, mode, 0, N, p("mesh.obj"), alpha, algorithm="cap", cap_finish="mesh")
    v, f = read_obj(p("mesh.obj"))
    assert np.array_equal(f, np.asarray(mesh.faces)) and np.array_equal(v, np.asarray(mesh.vertices))
    assert 0 < len(f) <= len(soup.faces) and len(v) < len(soup.vertices) and same_direction_edges(f, len(v)) == 0
    cv, cf, _ = meshclean.clean_mesh(soup.vertices, soup.faces, fill_holes=False)
    assert cv.cpu().numpy().tobytes() == v.tobytes() and np.array_equal(meshclean.orient_faces(cv, cf).cpu().numpy(), f)
    t = T.topology(f, len(v), v)
    assert t["flipped_faces"] == 0
    # the filter keys: components below the largest one's size go
    biggest = int(t["n_faces"].max())
    kept = generate_mc.generate_mc(model, mode, 0, N, p("big.obj"), alpha, algorithm="cap", min_component_faces=biggest)
    assert len(kept.faces) == int(t["n_faces"][t["n_faces"] >= biggest].sum())
    ov, of_, _ = T.remove_small_components(v, f, min_faces=biggest)
    assert np.asarray(kept.vertices).tobytes() == ov.tobytes() and np.array_equal(np.asarray(kept.faces), of_)
    none = generate_mc.generate_mc(model, mode, 0, N, p("none.obj"), alpha, algorithm="cap", min_component_area_ratio=2.0)
    assert len(none.faces) == 0 and len(none.vertices) == 0
    sparse = generate_mc.generate_mc(model, mode, 0, N, p("sparse.obj"), alpha, algorithm="cap", sparse=True, cap_finish="mesh")
    assert np.array_equal(tri_set(sparse.vertices, sparse.faces), tri_set(v, f))
