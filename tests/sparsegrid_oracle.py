# coding: utf-8
"""numpy oracle of the brick-sparse narrow band (layout in include/dudf_hip.h): lattice indices, the selection
(candidate and stored bricks, slot table), gather / scatter between dense fields and brick storage, and which cells of a dense
field are active.  Written from the rules, not from the kernels: loops over bricks, no scans."""
import math

import numpy as np


def dims(N, B):
    """(m, nb, nl): cells per side, cell bricks per side, storage-lattice bricks per side."""
    m = N - 1
    return m, (m + B - 1) // B, m // B + 1


def lattice_indices(N, B):
    """Fine indices of the nb + 1 coarse lattice points of one axis."""
    m, nb, _ = dims(N, B)
    return np.minimum(np.arange(nb + 1) * B, m)


def bound(N, B, threshold, lipschitz):
    return threshold + lipschitz * (math.sqrt(3.0) / 2.0) * B * (2.0 / (N - 1))


def select(coarse, N, B, bnd):
    """coarse (nb+1,)*3 float32 -> (slot (nl,nl,nl) int32, stored ids, candidate ids), ids ascending int32 over the nl^3 lattice."""
    m, nb, nl = dims(N, B)
    coarse = np.asarray(coarse, dtype=np.float32).reshape(nb + 1, nb + 1, nb + 1)
    cand = np.zeros((nl, nl, nl), dtype=bool)
    for b0 in range(nb):
        for b1 in range(nb):
            for b2 in range(nb):
                c = coarse[b0:b0 + 2, b1:b1 + 2, b2:b2 + 2].astype(np.float64)
                cand[b0, b1, b2] = bool(np.isnan(c).any() or c.min() <= bnd)
    stored = np.zeros_like(cand)
    for b0, b1, b2 in np.argwhere(cand):
        stored[b0:min(b0 + 2, nl), b1:min(b1 + 2, nl), b2:min(b2 + 2, nl)] = True      # slicing clips b + delta to the lattice
    stored_ids = np.flatnonzero(stored.reshape(-1)).astype(np.int32)
    slot = np.full(nl ** 3, -1, dtype=np.int32)
    slot[stored_ids] = np.arange(len(stored_ids), dtype=np.int32)
    return slot.reshape(nl, nl, nl), stored_ids, np.flatnonzero(cand.reshape(-1)).astype(np.int32)


def brick_points(ids, N, B):
    """((S,B,B,B,3) clamped grid indices, (S,B,B,B) in-grid mask) of the points of bricks `ids`."""
    m, _, nl = dims(N, B)
    ids = np.asarray(ids, dtype=np.int64)
    b = np.stack([ids // (nl * nl), (ids // nl) % nl, ids % nl], -1)                       # (S, 3)
    loc = np.stack(np.meshgrid(np.arange(B), np.arange(B), np.arange(B), indexing="ij"), -1)  # (B,B,B,3)
    g = b[:, None, None, None, :] * B + loc[None]
    return np.minimum(g, m), (g <= m).all(-1)


def gather(ndf, vec, stored_ids, N, B):
    """Dense (N,N,N), (N,N,N,3) -> brick storage (S,B,B,B), (S,B,B,B,3); padding holds the value at the clamped index."""
    g, _ = brick_points(stored_ids, N, B)
    return ndf[g[..., 0], g[..., 1], g[..., 2]], vec[g[..., 0], g[..., 1], g[..., 2]]


def scatter(df, vec, stored_ids, N, B, fill=np.nan):
    g, ok = brick_points(stored_ids, N, B)
    ndf = np.full((N, N, N), fill, dtype=np.float32); v = np.full((N, N, N, 3), fill, dtype=np.float32)
    ndf[g[ok][:, 0], g[ok][:, 1], g[ok][:, 2]] = df[ok]
    v[g[ok][:, 0], g[ok][:, 1], g[ok][:, 2]] = vec[ok]
    return ndf, v


def active_cells(ndf, threshold):
    """(m,m,m) bool: min over the cell's 8 corners <= threshold (float64 comparison, NaN: not active — the extractor's test)."""
    d = np.asarray(ndf, dtype=np.float64)
    m = d.shape[0] - 1
    mn = np.full((m, m, m), np.inf)
    nan = np.zeros((m, m, m), dtype=bool)
    for c in range(8):
        s = d[(c & 1):(c & 1) + m, ((c >> 1) & 1):((c >> 1) & 1) + m, ((c >> 2) & 1):((c >> 2) & 1) + m]
        nan |= np.isnan(s)
        mn = np.minimum(mn, np.where(np.isnan(s), np.inf, s))
    return (mn <= threshold) & ~nan


def candidate_cell_mask(candidate_ids, N, B):
    """(m,m,m) bool: the cells the candidate bricks hold."""
    m, _, nl = dims(N, B)
    mask = np.zeros((m, m, m), dtype=bool)
    for b in np.asarray(candidate_ids, dtype=np.int64):
        b0, b1, b2 = b // (nl * nl), (b // nl) % nl, b % nl
        mask[b0 * B:(b0 + 1) * B, b1 * B:(b1 + 1) * B, b2 * B:(b2 + 1) * B] = True
    return mask
