# coding: utf-8
"""numpy restatement of the mesh clean-up rules of DESIGN.md §3 (`diffudf_amd.meshclean`, csrc/dudf_meshclean.hip): test
infrastructure only.  Vertices (V,3) float64, faces (F,3) int64; every function returns new arrays.

round(v, f)       drop invalid faces, weld, remap, prune (degenerate, then duplicate), compact
fill_holes(v, f)  close the 3- and 4-edge holes of a round's result
clean(v, f)       round, fill_holes, rounds until (V, F) stops changing
border_edges      the (E,2) undirected edges used by exactly one face, ascending
smooth            Jacobi Laplacian smoothing of the border vertices, neighbours summed in ascending index order"""
import numpy as np

COUNT_NAMES = ("vertices", "faces", "welded", "unreferenced", "duplicate_faces", "degenerate_faces", "holes3", "holes4",
               "invalid_faces")
_KMAX = 9223372036854774784.0                       # the largest double below 2^63


def vertex_keys(v, digits=8):
    """rint(v * 10^digits) per coordinate (one double multiply, half to even) as int64, saturated at the ends of int64."""
    with np.errstate(over="ignore", invalid="ignore"):
        k = np.rint(np.asarray(v, np.float64) * float(10 ** digits))
    return np.clip(k, -9223372036854775808.0, _KMAX).astype(np.int64)


def degenerate(p0, p1, p2):
    """longest edge L <= 1e-8 or |(p1 - p0) x (p2 - p0)| / L <= 1e-8, compared squared: L^2 <= 1e-16 or |c|^2 <= 1e-16 L^2 — sums
    left to right, no contraction, no square root and no division."""
    with np.errstate(all="ignore"):
        a, b, e = p1 - p0, p2 - p0, p2 - p1
        sq = lambda u: (u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]   # noqa: E731
        l2 = np.maximum(np.maximum(sq(a), sq(e)), sq(b))
        c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                      a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
        return (l2 <= 1e-16) | (sq(c) <= 1e-16 * l2)


def round_parts(v, f, digits=8):
    """One round without the compaction: (rep (V,) int64 with -1 for vertices no valid face uses, g (F,3) remapped faces,
    state (F,) 0 invalid / 1 degenerate / 2 duplicate / 3 alive)."""
    v = np.asarray(v, np.float64).reshape(-1, 3); f = np.asarray(f, np.int64).reshape(-1, 3)
    V, F = len(v), len(f)
    state = np.zeros(F, np.int64)
    inr = ((f >= 0) & (f < V)).all(1)
    valid = inr.copy()
    valid[inr] &= np.isfinite(v).all(1)[f[inr]].all(1)
    rep = np.full(V, -1, np.int64)
    idx = np.unique(f[valid])
    if len(idx):
        _, inv = np.unique(vertex_keys(v[idx], digits), axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        first = np.full(inv.max() + 1, V, np.int64)
        np.minimum.at(first, inv, idx)
        rep[idx] = first[inv]
    g = np.full((F, 3), -1, np.int64)
    g[valid] = rep[f[valid]]
    vi = np.nonzero(valid)[0]
    deg = degenerate(v[g[vi, 0]], v[g[vi, 1]], v[g[vi, 2]])
    state[vi[deg]] = 1
    rest = vi[~deg]
    _, first = np.unique(np.sort(g[rest], axis=1), axis=0, return_index=True)
    state[rest] = 2
    state[rest[first]] = 3
    return rep, g, state


def _compact(v, rep, g, state, extra=None):
    V = len(v)
    faces = g[state == 3]
    if extra is not None and len(extra):
        faces = np.concatenate([faces, extra])
    keep = np.zeros(V, bool)
    keep[faces.reshape(-1)] = True
    new = np.cumsum(keep) - 1
    n_ref = int((rep >= 0).sum()); n_rep = int((rep == np.arange(V)).sum())
    counts = dict(vertices=int(keep.sum()), faces=len(faces), welded=n_ref - n_rep, unreferenced=V - (n_ref - n_rep) - int(keep.sum()),
                  duplicate_faces=int((state == 2).sum()), degenerate_faces=int((state == 1).sum()), holes3=0, holes4=0,
                  invalid_faces=int((state == 0).sum()))
    return v[keep].copy(), new[faces].reshape(-1, 3), counts


def round(v, f, digits=8):                                  # noqa: A001 (the issue's name)
    v = np.asarray(v, np.float64).reshape(-1, 3)
    rep, g, state = round_parts(v, f, digits)
    return _compact(v, rep, g, state)


def _edge_table(f, V):
    """(keys u * V + w of the undirected edges u < w, their use counts, sorted keys of the directed edges); u == w is no edge."""
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]]); b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    m = a != b
    a, b = a[m], b[m]
    und, cnt = np.unique(np.minimum(a, b) * V + np.maximum(a, b), return_counts=True)
    return und, cnt, np.unique(a * V + b)


def border_edges(f, n_vertices):
    """(E,2) int64: the undirected edges (u < w) that exactly one face uses, ascending.  Faces with an index outside [0, V) are
    skipped."""
    f = np.asarray(f, np.int64).reshape(-1, 3); V = int(n_vertices)
    f = f[((f >= 0) & (f < V)).all(1)]
    und, cnt, _ = _edge_table(f, max(V, 1))
    k = und[cnt == 1]
    return np.stack([k // max(V, 1), k % max(V, 1)], 1)


def hole_faces(f, V):
    """The faces that close the 3- and 4-edge holes of faces `f` over V vertices, holes in ascending smallest vertex:
    (new faces (K,3), number of 3-holes, number of 4-holes)."""
    f = np.asarray(f, np.int64).reshape(-1, 3)
    if len(f) == 0:
        return np.zeros((0, 3), np.int64), 0, 0
    und, cnt, directed = _edge_table(f, V)
    k = und[cnt == 1]
    u, w = k // V, k % V
    deg = np.bincount(np.concatenate([u, w]), minlength=V)
    src = np.concatenate([u, w]); dst = np.concatenate([w, u])
    order = np.lexsort((dst, src))
    src, dst = src[order], dst[order]
    start = np.searchsorted(src, np.arange(V))
    out, n3, n4 = [], 0, 0
    for a in np.nonzero(deg == 2)[0]:
        b, d = int(dst[start[a]]), int(dst[start[a] + 1])
        cyc, prev, cur = [int(a)], int(a), b
        while len(cyc) < 5 and cur != a and cur > a and deg[cur] == 2:
            cyc.append(cur)
            n0, n1 = int(dst[start[cur]]), int(dst[start[cur] + 1])
            prev, cur = cur, (n1 if n0 == prev else n0)
        if cur != a or len(cyc) not in (3, 4):
            continue
        rev = np.searchsorted(directed, a * V + b) < len(directed) and directed[np.searchsorted(directed, a * V + b)] == a * V + b
        new = [(a, b, d)] if len(cyc) == 3 else [(a, b, cyc[2]), (cyc[2], d, a)]
        assert cyc[-1] == d
        out += [t[::-1] for t in new] if rev else new
        n3 += len(cyc) == 3; n4 += len(cyc) == 4
    return np.array(out, np.int64).reshape(-1, 3), n3, n4


def fill_holes(v, f):
    f = np.asarray(f, np.int64).reshape(-1, 3)
    new, _, _ = hole_faces(f, len(v))
    return np.asarray(v, np.float64).copy(), np.concatenate([f, new])


def round_fill(v, f, digits=8):
    """A round whose result has its holes filled: what one device count / emit pair with fill_holes does."""
    v = np.asarray(v, np.float64).reshape(-1, 3)
    rep, g, state = round_parts(v, f, digits)
    new, n3, n4 = hole_faces(g[state == 3], len(v))
    vo, fo, counts = _compact(v, rep, g, state, new)
    counts["holes3"], counts["holes4"] = n3, n4
    return vo, fo, counts


def clean(v, f, fill=True, max_rounds=10, digits=8):
    """(vertices, faces, info): info sums the per-round counts (vertices / faces are those of the result) and adds `rounds`."""
    total = None
    rounds = 0
    while True:
        n = (len(v), len(f))
        v, f, c = round_fill(v, f, digits) if (fill and rounds == 0) else round(v, f, digits)
        rounds += 1
        total = c if total is None else {k: (c[k] if k in ("vertices", "faces") else total[k] + c[k]) for k in c}
        if rounds > 1 and (len(v), len(f)) == n:
            break
        if rounds > max_rounds:
            break
    total["rounds"] = rounds
    return v, f, total


def smooth(v, f, iterations=5, lam=0.3):
    """Jacobi smoothing of the border vertices: v += lam * (mean(border neighbours) - v), the sum starting at 0.0 and taking the
    neighbours in ascending index order, every average from the positions before the iteration."""
    v = np.asarray(v, np.float64).reshape(-1, 3).copy()
    e = border_edges(f, len(v))
    if len(e) == 0:
        return v
    src = np.concatenate([e[:, 0], e[:, 1]]); dst = np.concatenate([e[:, 1], e[:, 0]])
    order = np.lexsort((dst, src))
    src, dst = src[order], dst[order]
    deg = np.bincount(src, minlength=len(v))
    start = np.concatenate([[0], np.cumsum(deg)[:-1]])
    bv = np.nonzero(deg)[0]
    for _ in range(int(iterations)):
        s = np.zeros((len(bv), 3))
        for j in range(int(deg.max())):
            m = deg[bv] > j
            s[m] = s[m] + v[dst[start[bv[m]] + j]]
        with np.errstate(all="ignore"):
            mean = s / deg[bv][:, None].astype(np.float64)
            new = v[bv] + lam * (mean - v[bv])
        v = v.copy(); v[bv] = new
    return v
