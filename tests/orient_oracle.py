# coding: utf-8
"""numpy oracle of the K-nearest search and the normal orientation (csrc/dudf_orient.hip), and the clouds their
tests share.  Pinned by tests/test_orient_cpu.py."""
import numpy as np

U = 2.0 ** -24


# ---- K nearest neighbours ---------------------------------------------------------------------------------------------------------
def pair_distance(x, y):
    """float64 squared distances of the fp32 rows x[i], y[i] from the differences (never |x|^2 + |y|^2 - 2 x.y)."""
    d = np.asarray(x, dtype=np.float32).astype(np.float64) - np.asarray(y, dtype=np.float32).astype(np.float64)
    return (d * d).sum(axis=-1)


def _smallest_exact(d, K):
    """(values, columns) (rows, K): the K smallest entries of every row of d by (value, column), ties included, without sorting rows:
    everything below the K-th smallest value, then the first columns that equal it."""
    rows, m = d.shape
    k = min(K, m)
    v = np.partition(d, k - 1, axis=1)[:, k - 1:k]
    below = d < v
    room = k - below.sum(axis=1, keepdims=True)
    equal = d == v
    keep = below | (equal & (np.cumsum(equal, axis=1) <= room))
    r, c = np.nonzero(keep)                                       # row-major: columns ascending inside a row, exactly k per row
    cols = c.reshape(rows, k)
    vals = np.take_along_axis(d, cols, axis=1)
    o = np.lexsort((cols, vals), axis=1)
    return np.take_along_axis(vals, o, axis=1), np.take_along_axis(cols, o, axis=1)


def knn(x, y, K, exclude_self=False, chunk=512, exact=None):
    """(dist (n,K) float64, idx (n,K) int64): the K rows of y nearest to every row of x, float64 arithmetic on the fp32 inputs,
    ascending by (distance, index); fewer than K candidates: +inf / -1.  Rows of y with a NaN or an infinity are no candidates.
    exact (the default up to m = 4096): every distance from the differences, ties across the K-th place resolved by index.
    Otherwise K + 8 candidates by the matmul form, whose error (~1e-15) is far below the gaps of the clouds it is used on, then the
    exact distances of those; a tie across the candidate boundary raises."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64); y = np.asarray(y, dtype=np.float32).astype(np.float64)
    n, m = len(x), len(y)
    dist = np.full((n, K), np.inf); idx = np.full((n, K), -1, dtype=np.int64)
    ok = np.isfinite(y).all(axis=1)
    if exact is None:
        exact = m <= 4096
    cand = min(m, K + 8)
    yy = (y * y).sum(axis=1)
    for a in range(0, n, chunk):
        xs = x[a:a + chunk]
        rows = np.arange(a, a + len(xs))
        with np.errstate(all="ignore"):
            if exact:
                d = ((xs[:, 0:1] - y[None, :, 0]) ** 2 + (xs[:, 1:2] - y[None, :, 1]) ** 2) + (xs[:, 2:3] - y[None, :, 2]) ** 2
            else:
                d = (xs * xs).sum(axis=1)[:, None] + yy[None, :] - 2.0 * (xs @ y.T)
        d[:, ~ok] = np.inf
        d[np.isnan(d)] = np.inf                                   # a non-finite row of x has no candidates
        if exclude_self:
            inside = rows < m
            d[np.nonzero(inside)[0], rows[inside]] = np.inf
        if exact:
            dd, order = _smallest_exact(d, K)
        else:
            part = np.argpartition(d, cand - 1, axis=1)[:, :cand]
            approx = np.take_along_axis(d, part, axis=1)
            far = approx.max(axis=1)
            dd = ((xs[:, None, :] - y[part]) ** 2).sum(axis=2)
            dd[approx == np.inf] = np.inf
            o = np.lexsort((part, dd), axis=1)
            part = np.take_along_axis(part, o, axis=1); dd = np.take_along_axis(dd, o, axis=1)
            if cand < m and (dd[:, min(K, cand) - 1] >= far * (1 - 1e-9)).any():
                raise AssertionError("knn oracle: the candidate set is too small for this cloud")
            order, dd = part[:, :K], dd[:, :K]
        k = order.shape[1]
        good = np.isfinite(dd)
        dist[a:a + len(xs), :k] = np.where(good, dd, np.inf)
        idx[a:a + len(xs), :k] = np.where(good, order, -1)
    return dist, idx


# ---- orientation ---------------------------------------------------------------------------------------------------------------------
def edge_keys(normals, idx):
    """(keys uint64, i, j, sign) of the valid slots: key = bits of w << 32 | slot, w = 1 - |dot| and dot = (nx nx' + ny ny') + nz nz' in
    fp32 without contraction — every numpy operation on float32 arrays rounds once, as the device does."""
    nrm = np.ascontiguousarray(normals, dtype=np.float32)
    idx = np.asarray(idx, dtype=np.int64)
    n, K = idx.shape
    assert n * K < 2 ** 32
    e = np.arange(n * K, dtype=np.int64)
    i = e // K
    j = idx.reshape(-1)
    valid = (j >= 0) & (j < n) & (j != i)
    e, i, j = e[valid], i[valid], j[valid]
    with np.errstate(all="ignore"):
        dot = (nrm[i, 0] * nrm[j, 0] + nrm[i, 1] * nrm[j, 1]) + nrm[i, 2] * nrm[j, 2]
        w = np.float32(1.0) - np.abs(dot)
    assert dot.dtype == np.float32 and w.dtype == np.float32
    keys = (w.view(np.uint32).astype(np.uint64) << np.uint64(32)) | e.astype(np.uint64)
    return keys, i, j, dot < 0


def z_code(z):
    """Order-preserving uint32 code of fp32 z (after -0 -> +0): the seed of a component is the largest (code, -index)."""
    b = (np.asarray(z, dtype=np.float32) + np.float32(0.0)).view(np.uint32)
    return np.where(b >> np.uint32(31), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def orient(points, normals, idx):
    """dict(normals, flip uint8, component int64, components, forest_edges): Kruskal over the sorted keys (the key is a strict
    total order, so the minimum spanning forest is unique) with a union-find that carries the flip parity to the parent; per
    component the seed (largest z, smallest index) is flipped iff its n_z < 0 and every vertex follows from its parity to the seed."""
    pts = np.asarray(points, dtype=np.float32); nrm = np.ascontiguousarray(normals, dtype=np.float32)
    n = len(pts)
    keys, ei, ej, sign = edge_keys(nrm, idx)
    order = np.argsort(keys, kind="stable")
    parent = list(range(n)); par = [0] * n

    def find(v):
        path = []
        while parent[v] != v:
            path.append(v); v = parent[v]
        acc = 0
        for u in reversed(path):                 # parity to the root, from the vertex next to the root outwards
            acc ^= par[u]
            parent[u] = v; par[u] = acc
        return v

    edges = 0
    for a, b, s in zip(ei[order].tolist(), ej[order].tolist(), sign[order].tolist()):
        ra, rb = find(a), find(b)
        if ra == rb:
            continue
        parent[ra] = rb; par[ra] = par[a] ^ par[b] ^ int(s)
        edges += 1
    root = np.array([find(v) for v in range(n)], dtype=np.int64)
    parity = np.array(par, dtype=np.uint8)
    parity[root == np.arange(n)] = 0
    code = z_code(pts[:, 2]).astype(np.uint64)
    seed_key = (code << np.uint64(32)) | (np.uint64(0xffffffff) - np.arange(n, dtype=np.uint64))
    best = np.zeros(n, dtype=np.uint64); np.maximum.at(best, root, seed_key)
    comp = np.full(n, n, dtype=np.int64); np.minimum.at(comp, root, np.arange(n))
    seed = (np.uint64(0xffffffff) - (best & np.uint64(0xffffffff))).astype(np.int64)      # per root; garbage elsewhere
    seed_of = seed[root]
    flip = parity ^ parity[seed_of] ^ (nrm[seed_of, 2] < 0).astype(np.uint8)
    out = np.where(flip[:, None].astype(bool), -nrm, nrm)
    return {"normals": out, "flip": flip.astype(np.uint8), "component": comp[root], "components": int((root == np.arange(n)).sum()),
            "forest_edges": edges}


def inconsistent(out_normals, true_normals, component):
    """Normals that disagree with true_normals up to one global sign per component."""
    agree = (np.asarray(out_normals, dtype=np.float64) * np.asarray(true_normals, dtype=np.float64)).sum(axis=1) > 0
    bad = 0
    for c in np.unique(component):
        a = agree[component == c]
        bad += int(min(a.sum(), len(a) - a.sum()))
    return bad


# ---- clouds --------------------------------------------------------------------------------------------------------------------------
def random_flips(normals):
    """The normals with independently random signs from default_rng(0)."""
    s = np.where(np.random.default_rng(0).random(len(normals)) < 0.5, -1.0, 1.0).astype(np.float32)
    return (np.asarray(normals, dtype=np.float32) * s[:, None]).astype(np.float32)


def sphere(n, radius=0.8, centre=(0.0, 0.0, 0.0), seed=1):
    """(points, outward unit normals) float32: n uniform points on a sphere."""
    g = np.random.default_rng(seed).normal(size=(n, 3))
    u = g / np.linalg.norm(g, axis=1, keepdims=True)
    return (u * radius + np.asarray(centre)).astype(np.float32), u.astype(np.float32)


def two_spheres(n_each=3000):
    a, na = sphere(n_each, 0.3, (-0.5, 0.0, 0.0), seed=2)
    b, nb = sphere(n_each, 0.3, (0.5, 0.0, 0.0), seed=3)
    return np.concatenate([a, b]), np.concatenate([na, nb])


def torus(n, R=0.6, r=0.2, seed=4):
    """(points, outward unit normals) float32 on a torus around the z axis."""
    rng = np.random.default_rng(seed)
    a, b = rng.random(n) * 2 * np.pi, rng.random(n) * 2 * np.pi
    nrm = np.stack([np.cos(b) * np.cos(a), np.cos(b) * np.sin(a), np.sin(b)], axis=1)
    pts = np.stack([R * np.cos(a), R * np.sin(a), np.zeros(n)], axis=1) + r * nrm
    return pts.astype(np.float32), nrm.astype(np.float32)


def polyline(n):
    """n points along a helix, each one's two nearest neighbours its predecessor and successor; normals = radial direction."""
    t = np.arange(n) * 0.05
    pts = np.stack([np.cos(t), np.sin(t), t * 0.02], axis=1)
    nrm = np.stack([np.cos(t), np.sin(t), np.zeros(n)], axis=1)
    return pts.astype(np.float32), nrm.astype(np.float32)


def lattice(side=12, scale=1.0 / 8.0):
    g = np.arange(side, dtype=np.float32) * np.float32(scale)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
