# coding: utf-8
"""numpy restatement of the mesh-topology rules of DESIGN.md §3.6b (`diffudf_amd.meshclean.face_topology`, csrc/dudf_meshtopo.hip), and
the meshes its tests share: test infrastructure only.  Pinned by tests/test_meshtopo_cpu.py.

Rules.  faces (F,3) int64, V vertices, optionally vertices (V,3) float64.
  - a face is IGNORED if an index lies outside [0, V) or two of its indices are equal: never dereferenced, no edge, its own component,
    flip 0, counted;
  - every other face uses its three directed edges (a,b), (b,c), (c,a) under the undirected key (min << 32) | max.  A key with one use
    is a BORDER edge; with two uses MANIFOLD: it links the two faces, with sign s = 1 iff both traverse it in the same direction; with
    more NON-MANIFOLD: counted, links nothing.  (A duplicated face shares three manifold edges with its twin.)
  - FOREST: the minimum spanning forest of the face graph under the key (each key is one link: the order is strict, the forest unique),
    here by Kruskal over the ascending keys with a union-find that carries the flip parity (the shape of tests/orient_oracle.py);
  - the component LABEL of a face is the smallest face index of its component; that face keeps its winding and every other face's
    flip is its parity relative to it along the forest.  A flipped face (a,b,c) is written (a,c,b);
  - INCONSISTENT edges: manifold edges both faces still traverse the same way after the flips (a non-orientable component);
  - AREA (with vertices): per non-ignored face nn = sqrt((n0 n0 + n1 n1) + n2 n2) of n = (b - a) x (c - a) (tests/surface_oracle.py's
    expression), q = uint64(rint(min(nn, 16) * 2^30)), a non-finite nn gives 0; a component's area_q is the integer sum, its area
    area_q * 2^-31;
  - counts, in this order: components (ignored faces included), forest_edges, manifold_edges, border_edges, nonmanifold_edges,
    ignored_faces, flipped_faces, inconsistent_edges.
Filter: a component stays iff n_faces >= min_faces, area_q >= ceil(min_area * 2^31) and area_q >= ceil(min_area_ratio * sum(area_q)) —
integer comparisons —; keep_largest = k then keeps the k largest of those by (area_q, n_faces) descending, ties to the smaller label.
Submesh of a face mask: kept faces in their order (a kept face with an index outside [0, V) goes), the vertices they use in their
order, faces re-indexed."""
import math

import numpy as np

COUNT_NAMES = ("components", "forest_edges", "manifold_edges", "border_edges", "nonmanifold_edges", "ignored_faces", "flipped_faces",
               "inconsistent_edges")


def valid_faces(f, V):
    return ((f >= 0) & (f < V)).all(1) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])


def edge_uses(f, V):
    """(keys uint64 ascending-stable, face-slot ids e = 3 f + c in that order, forward: the use runs min -> max) of the valid faces."""
    ok = np.nonzero(valid_faces(f, V))[0]
    a = f[ok].reshape(-1)                                              # slot c of face: index c -> index (c + 1) % 3
    b = f[ok][:, [1, 2, 0]].reshape(-1)
    e = (3 * ok[:, None] + np.arange(3)[None, :]).reshape(-1)
    keys = (np.minimum(a, b).astype(np.uint64) << np.uint64(32)) | np.maximum(a, b).astype(np.uint64)
    order = np.argsort(keys, kind="stable")
    return keys[order], e[order], (a < b)[order]


def manifold_links(f, V):
    """(fa, fb, same, n_border, n_nonmanifold): the links in ascending key order."""
    keys, e, fwd = edge_uses(f, V)
    if len(keys) == 0:
        z = np.zeros(0, np.int64)
        return z, z, np.zeros(0, bool), 0, 0
    start = np.nonzero(np.concatenate([[True], keys[1:] != keys[:-1]]))[0]
    count = np.diff(np.concatenate([start, [len(keys)]]))
    two = start[count == 2]
    return e[two] // 3, e[two + 1] // 3, fwd[two] == fwd[two + 1], int((count == 1).sum()), int((count > 2).sum())


def face_area_q(v, f, ok):
    q = np.zeros(len(f), np.uint64)
    if v is None or not ok.any():
        return q
    a, b, c = v[f[ok, 0]], v[f[ok, 1]], v[f[ok, 2]]
    with np.errstate(all="ignore"):
        e, g = b - a, c - a
        n0 = e[:, 1] * g[:, 2] - e[:, 2] * g[:, 1]
        n1 = e[:, 2] * g[:, 0] - e[:, 0] * g[:, 2]
        n2 = e[:, 0] * g[:, 1] - e[:, 1] * g[:, 0]
        nn = np.sqrt((n0 * n0 + n1 * n1) + n2 * n2)
        fin = np.isfinite(nn)
        q[ok] = np.where(fin, np.rint(np.minimum(np.where(fin, nn, 0.0), 16.0) * 1073741824.0), 0.0).astype(np.uint64)
    return q


def topology(faces, n_vertices, vertices=None):
    """dict: faces (oriented), component, flip uint8, component_faces (F,) int64 and component_area_q (F,) uint64 (non-zero at label
    positions only), labels (C,) ascending, n_faces (C,), area_q (C,) uint64 / area (C,) float64 (None without vertices), and the
    eight counts by name."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V, F = int(n_vertices), len(f)
    assert 6 * F < 2 ** 32
    v = None if vertices is None else np.asarray(vertices, np.float64).reshape(-1, 3)
    ok = valid_faces(f, V)
    fa, fb, same, n_border, n_fin = manifold_links(f, V)
    parent = list(range(F)); par = [0] * F

    def find(x):
        path = []
        while parent[x] != x:
            path.append(x); x = parent[x]
        acc = 0
        for u in reversed(path):                 # parity to the root, from the face next to the root outwards
            acc ^= par[u]
            parent[u] = x; par[u] = acc
        return x

    forest = 0
    for a, b, s in zip(fa.tolist(), fb.tolist(), same.tolist()):
        ra, rb = find(a), find(b)
        if ra == rb:
            continue
        parent[ra] = rb; par[ra] = par[a] ^ par[b] ^ int(s)
        forest += 1
    root = np.array([find(x) for x in range(F)], dtype=np.int64)
    parity = np.array(par, dtype=np.uint8).reshape(F)
    parity[root == np.arange(F)] = 0
    lab_of_root = np.full(F, F, np.int64)
    np.minimum.at(lab_of_root, root, np.arange(F))
    comp = lab_of_root[root]
    flip = (parity ^ parity[comp]).astype(np.uint8) if F else np.zeros(0, np.uint8)
    out = f.copy()
    fl = flip.astype(bool)
    out[fl, 1], out[fl, 2] = f[fl, 2], f[fl, 1]
    nfaces = np.bincount(comp, minlength=F).astype(np.int64)
    q = face_area_q(v, f, ok)
    area_q = np.zeros(F, np.uint64)
    np.add.at(area_q, comp, q)
    labels = np.nonzero(nfaces)[0]
    bad = int((same ^ fl[fa] ^ fl[fb]).sum()) if len(fa) else 0
    res = {"faces": out, "component": comp, "flip": flip, "component_faces": nfaces, "component_area_q": area_q, "labels": labels,
           "n_faces": nfaces[labels], "area_q": None if v is None else area_q[labels],
           "area": None if v is None else area_q[labels].astype(np.float64) * 2.0 ** -31}
    res.update(zip(COUNT_NAMES, (len(labels), forest, len(fa), n_border, n_fin, int((~ok).sum()), int(fl.sum()), bad)))
    return res


def component_filter(labels, n_faces, area_q, min_faces=0, min_area=0.0, min_area_ratio=0.0, keep_largest=None):
    """(C,) bool, Python integers throughout."""
    q = [int(x) for x in area_q] if area_q is not None else [0] * len(labels)
    n = [int(x) for x in n_faces]
    t_area = math.ceil(float(min_area) * 2147483648.0)
    t_ratio = math.ceil(float(min_area_ratio) * float(sum(q)))
    keep = [n[i] >= min_faces and q[i] >= t_area and q[i] >= t_ratio for i in range(len(n))]
    if keep_largest is not None:
        cand = [(-q[i], -n[i], int(labels[i]), i) for i in range(len(n)) if keep[i]]
        keep = [False] * len(n)
        for *_, i in sorted(cand)[:max(int(keep_largest), 0)]:
            keep[i] = True
    return np.array(keep, dtype=bool)


def submesh(vertices, faces, keep):
    """(vertices, faces, (V', F'))."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3); f = np.asarray(faces, np.int64).reshape(-1, 3)
    k = np.asarray(keep).astype(bool) & ((f >= 0) & (f < len(v))).all(1)
    ff = f[k]
    use = np.zeros(len(v), bool)
    use[ff.reshape(-1)] = True
    new = np.cumsum(use) - 1
    return v[use].copy(), new[ff].reshape(-1, 3), (int(use.sum()), len(ff))


def remove_small_components(vertices, faces, **kw):
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    t = topology(faces, len(v), v)
    keep_c = component_filter(t["labels"], t["n_faces"], t["area_q"], **kw)
    by_label = np.zeros(max(len(t["faces"]), 1), bool)
    by_label[t["labels"][keep_c]] = True
    return submesh(v, t["faces"], by_label[t["component"]])


# ---- meshes ------------------------------------------------------------------------------------------------------------------------
def scramble(faces, seed, flips=True, permute=True):
    """The faces with random windings reversed and in a random order, from default_rng(seed)."""
    rng = np.random.default_rng(seed)
    f = np.asarray(faces, np.int64).copy()
    if flips:
        r = rng.random(len(f)) < 0.5
        f[r] = f[r][:, [0, 2, 1]]
    if permute:
        f = f[rng.permutation(len(f))]
    return f


def strip(n_faces):
    """(vertices, faces): a consistently wound triangle strip of n_faces faces in the plane z = 0: one chain of n_faces - 1 manifold
    edges."""
    n = n_faces + 2
    i = np.arange(n)
    v = np.stack([(i // 2).astype(np.float64), (i % 2).astype(np.float64), np.zeros(n)], 1)
    k = np.arange(n_faces)
    f = np.stack([k, k + 1, k + 2], 1)
    odd = k % 2 == 1
    f[odd] = f[odd][:, [1, 0, 2]]
    return v, f.astype(np.int64)


def mobius(n=12):
    """A Möbius band of 2 n faces: a strip of n quads around a circle whose last quad joins the first with the two rails swapped."""
    t = np.arange(n) * 2 * np.pi / n
    c = np.stack([np.cos(t), np.sin(t), np.zeros(n)], 1)
    w = 0.3 * np.stack([np.cos(t / 2) * np.cos(t), np.cos(t / 2) * np.sin(t), np.sin(t / 2)], 1)
    v = np.concatenate([c - w, c + w])                                 # rail 0: 0 .. n-1, rail 1: n .. 2n-1
    f = []
    for i in range(n):
        a0, a1 = i, n + i
        b0, b1 = (i + 1, n + i + 1) if i + 1 < n else (n, 0)           # the twist: rail 0 continues on rail 1
        f += [[a0, b0, a1], [b0, b1, a1]]
    return v, np.array(f, np.int64)


def grid_plane(nx=64, ny=64):
    """(vertices, faces): (nx + 1) x (ny + 1) lattice vertices, 2 nx ny consistently wound faces."""
    gx, gy = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="ij")
    v = np.stack([gx.reshape(-1) / nx, gy.reshape(-1) / ny, np.zeros(gx.size)], 1).astype(np.float64)
    idx = lambda i, j: i * (ny + 1) + j   # noqa: E731
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    i, j = i.reshape(-1), j.reshape(-1)
    f = np.concatenate([np.stack([idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)], 1), np.stack([idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)], 1)])
    return v, f.astype(np.int64)


TETRA_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64)
TETRA_F = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int64)          # outward


def tetrahedra(k, seed=7):
    """k disjoint tetrahedra of different sizes (areas differ), outward wound."""
    rng = np.random.default_rng(seed)
    s = 0.05 + 0.2 * rng.random(k)
    v = np.concatenate([TETRA_V * s[i] + np.array([i % 32, (i // 32) % 32, i // 1024], np.float64) for i in range(k)])
    f = np.concatenate([TETRA_F + 4 * i for i in range(k)])
    return v, f


def fin():
    """Three faces on the edge 0-1: one non-manifold edge, three components."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1]], np.float64)
    return v, np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], np.int64)


_CAP = {}


def cap_welded(kind, n):
    """(vertices, faces) of the CAP-UDF oracle's soup on `analytic_fields(n, kind)` of tests/test_capudf.py (the reference's 0.008
    cut), welded by tests/meshclean_oracle.clean(fill=False); once per session."""
    if (kind, n) not in _CAP:
        from oracle import capudf_oracle as C
        import meshclean_oracle as M
        from test_capudf import analytic_fields
        ndf, vec = analytic_fields(n, kind)
        v, t, _ = C.extract_mesh_CAP(ndf, vec, n)
        vo, fo, _ = M.clean(v, t, fill=False)
        _CAP[(kind, n)] = (vo, fo)
    return _CAP[(kind, n)]
