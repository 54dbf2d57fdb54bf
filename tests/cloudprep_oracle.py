# coding: utf-8
"""numpy oracle of the normal estimation and the statistical outlier test (csrc/dudf_cloudprep.hip), and the clouds
their tests share.  Pinned by tests/test_cloudprep_cpu.py.  Every step is the device's expression in float64, in the device's order:
numpy rounds once per operation, as the kernels do (they are built without contraction)."""
import numpy as np

from orient_oracle import knn, sphere  # noqa: F401  (the searches and the sphere of the orientation tests)


# ---- the 3x3 solver ------------------------------------------------------------------------------------------------------------------
def jacobi_eigh3(H):
    """(lam (n,3) ascending, V (n,3,3) with V[:, i, j] = component i of v_j): csrc/dudf_eigh3.h restated row-wise — cyclic Jacobi on
    the LOWER triangle of H (n,3,3), at most 10 sweeps, a row stops when its off-diagonal mass is below 1e-34 of the diagonal's."""
    H = np.asarray(H, dtype=np.float64)
    n = len(H)
    A = np.empty((n, 3, 3))
    for i in range(3):
        for j in range(3):
            A[:, i, j] = H[:, max(i, j), min(i, j)]
    V = np.zeros((n, 3, 3)); V[:, [0, 1, 2], [0, 1, 2]] = 1.0
    live = np.ones(n, dtype=bool)
    with np.errstate(all="ignore"):
        for _ in range(10):
            off = A[:, 0, 1] * A[:, 0, 1] + A[:, 0, 2] * A[:, 0, 2] + A[:, 1, 2] * A[:, 1, 2]
            dia = A[:, 0, 0] * A[:, 0, 0] + A[:, 1, 1] * A[:, 1, 1] + A[:, 2, 2] * A[:, 2, 2]
            live &= ~((off <= 1e-34 * dia) | (off == 0.0))
            if not live.any():
                break
            for p, q in ((0, 1), (0, 2), (1, 2)):
                r = 3 - p - q
                apq = A[:, p, q].copy()
                m = live & (apq != 0.0)
                th = (A[:, q, q] - A[:, p, p]) / (2.0 * apq)
                t = np.where(th >= 0, 1.0, -1.0) / (np.abs(th) + np.sqrt(th * th + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                sn = t * c
                app, aqq, arp, arq = A[:, p, p].copy(), A[:, q, q].copy(), A[:, r, p].copy(), A[:, r, q].copy()
                A[:, p, p] = np.where(m, app - t * apq, app)
                A[:, q, q] = np.where(m, aqq + t * apq, aqq)
                A[:, p, q] = A[:, q, p] = np.where(m, 0.0, apq)
                A[:, r, p] = A[:, p, r] = np.where(m, c * arp - sn * arq, arp)
                A[:, r, q] = A[:, q, r] = np.where(m, sn * arp + c * arq, arq)
                vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
                V[:, :, p] = np.where(m[:, None], c[:, None] * vp - sn[:, None] * vq, vp)
                V[:, :, q] = np.where(m[:, None], sn[:, None] * vp + c[:, None] * vq, vq)
    lam = np.stack([A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]], axis=1)
    for i, j in ((0, 1), (1, 2), (0, 1)):
        s = lam[:, i] > lam[:, j]
        lam[s, i], lam[s, j] = lam[s, j].copy(), lam[s, i].copy()
        vi, vj = V[s, :, i].copy(), V[s, :, j].copy()
        V[s, :, i], V[s, :, j] = vj, vi
    return lam, V


# ---- normals -------------------------------------------------------------------------------------------------------------------------
def estimate_normals(points, idx, include_self=True):
    """dict(normals (n,3) float32, eigenvalues (n,3) float64 ascending, counts (n,) int32, cov (n,3,3) float64 symmetric, fallback
    (n,) bool).  The neighbourhood of row i: i itself with include_self, then the slots of idx[i] in slot order, a slot outside [0, n)
    or equal to i skipped.  Mean and covariance in float64, sums from 0.0 in neighbourhood order, divided by the size c.  The normal
    is the first eigenvector of jacobi_eigh3, normalised in float64, rounded once.  c < 3, an all-zero covariance or a non-finite
    coordinate: (0, 0, 1) and eigenvalues 0."""
    p = np.asarray(points, dtype=np.float32).astype(np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    n, K = idx.shape
    rows = np.arange(n)
    valid = (idx >= 0) & (idx < n) & (idx != rows[:, None])
    safe = np.where(valid, idx, 0)
    finite_pt = np.isfinite(p).all(axis=1)
    members = [(np.ones(n, dtype=bool), rows)] if include_self else []
    members += [(valid[:, s], safe[:, s]) for s in range(K)]
    with np.errstate(all="ignore"):
        total = np.zeros((n, 3)); c = np.zeros(n, dtype=np.int32); fin = np.ones(n, dtype=bool)
        for ok, j in members:
            total = np.where(ok[:, None], total + p[j], total)
            fin &= ~ok | finite_pt[j]
            c += ok
        mean = total / c[:, None].astype(np.float64)
        cov = np.zeros((n, 3, 3))
        for ok, j in members:
            d = p[j] - mean
            for a in range(3):
                for b in range(a + 1):
                    cov[:, a, b] = np.where(ok, cov[:, a, b] + d[:, a] * d[:, b], cov[:, a, b])
        cov /= c[:, None, None].astype(np.float64)
        for a in range(3):
            for b in range(a):
                cov[:, b, a] = cov[:, a, b]
        fallback = ~fin | (c < 3)
        cov[fallback] = 0.0
        fallback |= (cov == 0.0).all(axis=(1, 2))
        lam, V = jacobi_eigh3(cov)
        v = V[:, :, 0]
        length = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        nrm = v / length[:, None]
    nrm[fallback] = (0.0, 0.0, 1.0)
    lam[fallback] = 0.0
    return {"normals": nrm.astype(np.float32), "eigenvalues": lam, "counts": c, "cov": cov, "fallback": fallback}


# ---- outliers ------------------------------------------------------------------------------------------------------------------------
def outliers(knn_dist, std_ratio=2.0):
    """dict(mean_dist (n,) float64, mean, std, threshold, keep (n,) bool, kept_idx int64): knn_dist (n,K) float32 holds SQUARED
    distances; d_i = the mean of sqrt over the finite slots in slot order (+inf without one), mean / std = the population statistics
    of the finite d_i (std from the centred values), keep = d_i <= mean + std_ratio * std."""
    d = np.asarray(knn_dist, dtype=np.float32)
    n, K = d.shape
    fin = np.isfinite(d)
    with np.errstate(all="ignore"):
        s = np.zeros(n)
        for k in range(K):
            s = np.where(fin[:, k], s + np.sqrt(d[:, k].astype(np.float64)), s)
        c = fin.sum(axis=1)
        mean_dist = np.where(c > 0, s / c, np.inf)
        f = np.isfinite(mean_dist)
        mu = mean_dist[f].mean() if f.any() else np.nan
        sigma = np.sqrt(((mean_dist[f] - mu) ** 2).mean()) if f.any() else np.nan
        thr = mu + std_ratio * sigma
        keep = mean_dist <= thr
    return {"mean_dist": mean_dist, "mean": float(mu), "std": float(sigma), "threshold": float(thr), "keep": keep,
            "kept_idx": np.flatnonzero(keep).astype(np.int64)}


# ---- clouds --------------------------------------------------------------------------------------------------------------------------
N_CLOUD = 4099                                   # 16 workgroups of 256 and a partial one


def sheet(n=N_CLOUD, seed=11):
    """(points, unit normals with n_z > 0) float32: the open sheet z = 0.15 sin 3x cos 2y over [-0.8, 0.8]^2, uniform in (x, y)."""
    xy = np.random.default_rng(seed).uniform(-0.8, 0.8, size=(n, 2))
    x, y = xy[:, 0], xy[:, 1]
    z = 0.15 * np.sin(3 * x) * np.cos(2 * y)
    g = np.stack([-0.45 * np.cos(3 * x) * np.cos(2 * y), 0.30 * np.sin(3 * x) * np.sin(2 * y), np.ones(n)], axis=1)
    return np.stack([x, y, z], axis=1).astype(np.float32), (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)


def sheet_with_outliers(n=N_CLOUD, planted=40, seed=12):
    """(points, planted rows): the sheet with `planted` more points at |z| in [0.5, 0.9] above and below it, at random rows."""
    p, _ = sheet(n - planted)
    rng = np.random.default_rng(seed)
    q = np.stack([rng.uniform(-0.8, 0.8, planted), rng.uniform(-0.8, 0.8, planted),
                  rng.uniform(0.5, 0.9, planted) * np.where(rng.random(planted) < 0.5, -1.0, 1.0)], axis=1).astype(np.float32)
    order = rng.permutation(n)
    allp = np.concatenate([p, q])[order]
    return allp, np.sort(np.flatnonzero(order >= n - planted))


def lattice_plane(side=20, jitter=0.2, seed=13):
    """side^2 points of the plane z = 0.25 on a jittered square lattice of spacing 1/16 (no two neighbour distances equal)."""
    g = np.arange(side) / 16.0
    xy = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    xy = xy + np.random.default_rng(seed).uniform(-jitter, jitter, size=xy.shape) / 16.0
    return np.concatenate([xy, np.full((len(xy), 1), 0.25)], axis=1).astype(np.float32)
