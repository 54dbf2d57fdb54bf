# coding: utf-8
"""Oracle side of the occupancy tests: the crossing rule of `dudf_mesh_occupancy` (include/dudf_hip.h) restated in numpy fp64, by
brute force over every (point, triangle) pair, the small meshes the tests share, and the reference's marching loop against a mesh.

The rule, for the ray from p along +x and a triangle (v0, v1, v2) of fp32 vertices:
  * (p.y, p.z) lies in the triangle's closed (y, z) extent and max x >= p.x;
  * the projected area (v1 - v0) x (v2 - v0) in (y, z) is not zero;
  * the edge function of a directed edge a -> b is evaluated from the LOWER vertex to the HIGHER one, lexicographic on (y, z, x),
    E = (hi.y - lo.y)(p.z - lo.z) - (hi.z - lo.z)(p.y - lo.y), one fp64 rounding per operation, and negated if a is the higher one;
    the point is on the LEFT of a -> b when E >= 0 for a lower -> higher edge and when E < 0 otherwise (a zero belongs to the left of
    the lower -> higher direction); all three edges must agree;
  * the crossing's x = ((e1 x0 + e2 x1) + e0 x2) / ((e0 + e1) + e2) is > p.x."""
import numpy as np


def _before(a, b):
    """a, b (T,3): a precedes b lexicographically on (y, z, x); equal vertices count as ordered."""
    return np.where(a[:, 1] != b[:, 1], a[:, 1] < b[:, 1], np.where(a[:, 2] != b[:, 2], a[:, 2] < b[:, 2], a[:, 0] <= b[:, 0]))


def _edge(a, b, py, pz):
    """(signed value (Q,T), left (Q,T)) of the directed edges a -> b (T,3) for the points (py, pz) (Q,1)."""
    fwd = _before(a, b)
    lo, hi = np.where(fwd[:, None], a, b), np.where(fwd[:, None], b, a)
    ly, lz = lo[None, :, 1], lo[None, :, 2]
    e = (hi[None, :, 1] - ly) * (pz - lz) - (hi[None, :, 2] - lz) * (py - ly)
    left = np.where(fwd[None, :], e >= 0.0, ~(e >= 0.0))
    return np.where(fwd[None, :], e, -e), left


def crossings(points, tri, chunk=1024):
    """(count (Q,) int32, margin (Q,)): the number of triangles of tri (T,9) float32 the +x ray of every point (Q,3) float32 crosses
    (-1 for a NaN point), and the smallest |edge function| / |projected area| over the triangles whose box the ray meets (inf if
    none): how close the point's projection comes to an edge, relative to the triangle."""
    points = np.asarray(points, dtype=np.float32); tri = np.asarray(tri, dtype=np.float32)
    assert points.ndim == 2 and points.shape[1] == 3 and tri.ndim == 2 and tri.shape[1] == 9
    t64 = tri.astype(np.float64)
    v0, v1, v2 = t64[:, 0:3], t64[:, 3:6], t64[:, 6:9]
    ylo, yhi = t64[:, 1::3].min(axis=1), t64[:, 1::3].max(axis=1)
    zlo, zhi = t64[:, 2::3].min(axis=1), t64[:, 2::3].max(axis=1)
    xhi = t64[:, 0::3].max(axis=1)
    area2 = (v1[:, 1] - v0[:, 1]) * (v2[:, 2] - v0[:, 2]) - (v1[:, 2] - v0[:, 2]) * (v2[:, 1] - v0[:, 1])
    count = np.empty(len(points), dtype=np.int32); margin = np.empty(len(points))
    with np.errstate(all="ignore"):
        for s in range(0, len(points), chunk):
            p = points[s:s + chunk].astype(np.float64)
            px, py, pz = p[:, 0:1], p[:, 1:2], p[:, 2:3]
            box = (py >= ylo) & (py <= yhi) & (pz >= zlo) & (pz <= zhi) & (xhi >= px)
            e0, s0 = _edge(v0, v1, py, pz)
            e1, s1 = _edge(v1, v2, py, pz)
            e2, s2 = _edge(v2, v0, py, pz)
            total = (e0 + e1) + e2
            x = ((e1 * v0[None, :, 0] + e2 * v1[None, :, 0]) + e0 * v2[None, :, 0]) / total
            hit = box & (area2 != 0.0)[None, :] & (s0 == s1) & (s1 == s2) & (total != 0.0) & (x > px)
            c = hit.sum(axis=1).astype(np.int32)
            c[np.isnan(p).any(axis=1)] = -1
            count[s:s + chunk] = c
            rel = np.minimum(np.minimum(np.abs(e0), np.abs(e1)), np.abs(e2)) / np.abs(area2)[None, :]
            rel = np.where(box & (area2 != 0.0)[None, :], rel, np.inf)
            margin[s:s + chunk] = rel.min(axis=1) if rel.shape[1] else np.inf
    return count, margin


def cube(h=0.5):
    """(vertices (8,3), faces (12,3)) of the cube [-h, h]^3, outward orientation."""
    v = np.array([[x, y, z] for x in (-h, h) for y in (-h, h) for z in (-h, h)], dtype=np.float64)      # index = 4 ix + 2 iy + iz
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                  [1, 5, 7], [1, 7, 3]], dtype=np.int64)
    return v, f


def soup(v, f):
    return np.concatenate([v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]], axis=1).astype(np.float32)


def lattice(n=9, step=0.25):
    """(n^3, 3) float32 lattice points centred on the origin."""
    a = (np.arange(n) - (n - 1) / 2) * step
    return np.stack(np.meshgrid(a, a, a, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)


def cube_inside(p, h=0.5):
    """What the rule makes of the cube: the ray crosses the face x = +h when p.x < h and the face x = -h when p.x < -h, so the parity
    is odd for -h <= p.x < h; the footprint is the half-open square the tie rule defines: -h < y <= h, -h <= z < h."""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return (x >= -h) & (x < h) & (y > -h) & (y <= h) & (z >= -h) & (z < h)


def strip(T):
    """(T,9) float32: T triangles of a zig-zag strip tilted against all three axes — an OPEN mesh whose consecutive triangles share
    an edge."""
    k = np.arange(T + 2)
    v = np.stack([0.3 * np.sin(0.7 * k) + 0.02 * k, -0.9 + 1.8 * k / (T + 1), np.where(k % 2 == 0, -0.5, 0.5) + 0.05 * np.cos(1.3 * k)], axis=1)
    f = np.stack([k[:-2], k[1:-1], k[2:]], axis=1)
    f[1::2] = f[1::2, ::-1]                                       # a consistent orientation along the strip
    return soup(v, f)


def march(distance, rays, t0, mask_rays, surface_eps=0.001, max_iterations=30, bound=1.3):
    """The marching loop of the reference's ground-truth renderer (src/render_st.py:255-268) operation for operation, with
    `distance` ((n,3) float32 -> (n,) float32) in the place of `scene.compute_distance`.  t0 (M,3) float64 and mask_rays (M,) bool
    are updated in place.  Returns (hits, fragile): fragile marks the rays one of whose distances came within a relative 1e-6 of
    surface_eps, or one of whose coordinates within 1e-9 of +-bound — a last-bit difference could send those the other way."""
    hits = np.zeros_like(mask_rays, dtype=bool)
    fragile = np.zeros_like(mask_rays, dtype=bool)
    iteration = 0
    while np.sum(mask_rays) > 0 and iteration < max_iterations:
        udfs = np.expand_dims(np.asarray(distance(t0[mask_rays].astype(np.float32)), dtype=np.float32), -1)
        t0[mask_rays] += rays[mask_rays] * np.hstack([udfs, udfs, udfs])
        fragile[mask_rays] |= np.abs(udfs.squeeze(-1).astype(np.float64) - surface_eps) <= 1e-6 * surface_eps
        fragile[mask_rays] |= (np.abs(np.abs(t0[mask_rays]) - bound) <= 1e-9).any(axis=1)
        mask = udfs.squeeze(-1) < surface_eps
        hits[mask_rays] += mask
        mask_rays[mask_rays] *= np.logical_not(mask)
        mask_rays *= np.logical_and(np.all(t0 > -bound, axis=1), np.all(t0 < bound, axis=1))
        iteration += 1
    return hits, fragile
