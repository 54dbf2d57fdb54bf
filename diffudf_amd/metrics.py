# coding: utf-8
"""Chamfer distance and normal consistency on the device — the part of `pytorch3d.loss.chamfer_distance` that reference
cuantitative.py:10-19 uses (pytorch3d is a CUDA extension), and the vertex normals open3d computes for it at :99-100.

The nearest-neighbour search, the sums behind the means and the vertex normals are HIP kernels (csrc/dudf_chamfer.hip);
there is no CPU path: CPU tensors raise DudfError.

`knn_points` is the K > 1 half of pytorch3d's `knn_points` and `orient_normals` stands in for open3d's
`orient_normals_consistent_tangent_plane` (reference generate_pc.py:40); both are HIP kernels too (csrc/dudf_orient.hip).
`estimate_normals` and `remove_statistical_outliers` stand in for open3d's `estimate_normals` and `remove_statistical_outlier`, what
a raw scan needs before any of the above (csrc/dudf_cloudprep.hip).

`MeshIndex` / `mesh_distance` stand in for `o3d.t.geometry.RaycastingScene().add_triangles(...)` / `.compute_distance(...)`
(reference generate_df.py:108-110): the exact unsigned distance from points to a triangle mesh through a bounding-volume
hierarchy built and walked on the device (csrc/dudf_meshdist.hip).  `MeshIndex.occupancy` / `.signed_distance` are its
`compute_occupancy` / `compute_signed_distance` (src/dataset.py:35,50, src/render_st.py:275-276) and `.trace_rays` the marching loop
of src/render_st.py:255-268 as one kernel."""
import numpy as np
import torch

from . import hip_ops
from ._lib import DudfError


def nearest_points(x, y, norm=2):
    """(dist (n,) float32, idx (n,) int64): for every row of x (n,3) its nearest row of y (m,3) — the `dists[..., 0]` and
    `idx[..., 0]` of pytorch3d's `knn_points(x[None], y[None], norm=norm, K=1)`.  norm 2: squared Euclidean; norm 1: L1."""
    return hip_ops.nearest_points(x, y, norm)


def knn_points(x, y, K=1, exclude_self=False, brute=False):
    """(dists (n,K) float32, idx (n,K) int64): for every row of x (n,3) its K nearest rows of y (m,3) by squared Euclidean distance,
    nearest first (equal distances by index) — the `dists[0]` / `idx[0]` of pytorch3d's `knn_points(x[None], y[None], K=K)`.
    1 <= K <= 16.  exclude_self (for x is y): a point is not its own neighbour.  A row with fewer than K candidates is padded with
    +inf / -1.  The search walks a cell list built over y on the device; brute=True scans all of y (the same bits)."""
    return hip_ops.knn_points(x, y, K, exclude_self, brute)


def orient_normals(points, normals, k=10, return_info=False):
    """Normals (n,3) float32 with consistent signs — open3d's `orient_normals_consistent_tangent_plane(k)`: the k nearest
    neighbours of every point of the cloud, a minimum spanning forest of that graph under the weight 1 - |n_i . n_j|, signs
    propagated along it from the highest point of every connected component, which ends with n_z >= 0 (open3d joins
    the components with a Delaunay graph first, here each is seeded on its own).  With return_info also a dict: flip (n,) uint8,
    component (n,) int64, components, forest_edges, rounds, launches."""
    if not torch.is_tensor(points) or points.dim() != 2:
        raise DudfError("orient_normals: points must be an (n, 3) tensor")
    n = points.shape[0]
    if n == 0:
        out = hip_ops._tensor(normals, "orient_normals: normals", torch.float32, (3,), convert=True).clone()
        return (out, {"flip": torch.empty(0, dtype=torch.uint8, device=out.device), "component": torch.empty(0, dtype=torch.int64, device=out.device),
                      "components": 0, "forest_edges": 0, "rounds": 0, "launches": 0}) if return_info else out
    _, idx = hip_ops.knn_points(points, points, int(k), exclude_self=True, want_dist=False)
    out, flip, comp, counts, stats = hip_ops.orient_normals(points, normals, idx)
    if not return_info:
        return out
    c = counts.tolist()
    return out, {"flip": flip, "component": comp, "components": int(c[0]), "forest_edges": int(c[1]), **stats}


def estimate_normals(points, k=15, orient=True, orient_k=10, return_info=False):
    """Normals (n,3) float32 for a cloud that has none — open3d's `estimate_normals(KDTreeSearchParamKNN(k))` followed (orient=True)
    by `orient_normals_consistent_tangent_plane(orient_k)`: per point the direction of least variance of itself and its k nearest
    neighbours (fp64 covariance), then consistent signs.  ONE k-nearest search serves both steps when orient_k <= k:
    rows come nearest first, so the first orient_k columns are the orient_k-NN graph.  With return_info also a dict: eigenvalues
    (n,3) float64 ascending, counts (n,) int32 (neighbourhood sizes), and under "orient" the info dict of `orient_normals`."""
    points = hip_ops._tensor(points, "estimate_normals: points", torch.float32, (3,), convert=True)
    k, orient_k = int(k), int(orient_k)
    _, idx = hip_ops.knn_points(points, points, k, exclude_self=True, want_dist=False)
    normals, eig, cnt = hip_ops.estimate_normals(points, idx, include_self=True, want_info=return_info)
    info = {"eigenvalues": eig, "counts": cnt, "orient": None}
    if orient and points.shape[0] > 0:
        if orient_k <= k:
            oidx = idx[:, :orient_k].contiguous()
        else:
            _, oidx = hip_ops.knn_points(points, points, orient_k, exclude_self=True, want_dist=False)
        normals, flip, comp, counts, stats = hip_ops.orient_normals(points, normals, oidx, out=normals)
        if return_info:
            c = counts.tolist()
            info["orient"] = {"flip": flip, "component": comp, "components": int(c[0]), "forest_edges": int(c[1]), **stats}
    return (normals, info) if return_info else normals


def remove_statistical_outliers(points, nb_neighbors=16, std_ratio=2.0):
    """(kept_points (m,3), kept_index (m,) int64, info) — open3d's `remove_statistical_outlier(nb_neighbors, std_ratio)`: a point goes
    when its mean distance to its nb_neighbors nearest neighbours exceeds the cloud's mean of that quantity by more than std_ratio
    standard deviations.  info: mean, std, threshold (floats), removed (int), mean_dist (n,) float64, keep (n,)
    uint8.  The search, the statistics and the compaction run on the device; the count and the three statistics are read once."""
    points = hip_ops._tensor(points, "remove_statistical_outliers: points", torch.float32, (3,), convert=True)
    n = points.shape[0]
    if n == 0:
        return points, torch.empty(0, dtype=torch.int64, device=points.device), {
            "mean": float("nan"), "std": float("nan"), "threshold": float("nan"), "removed": 0,
            "mean_dist": torch.empty(0, dtype=torch.float64, device=points.device), "keep": torch.empty(0, dtype=torch.uint8, device=points.device)}
    dist, _ = hip_ops.knn_points(points, points, int(nb_neighbors), exclude_self=True, want_idx=False)
    mean_dist, keep, stats, kept, counts = hip_ops.cloud_outliers(dist, std_ratio)
    m = int(counts.item())
    s = stats.tolist()
    kept = kept[:m]
    return points[kept], kept, {"mean": s[0], "std": s[1], "threshold": s[2], "removed": n - m, "mean_dist": mean_dist, "keep": keep}


def _batched(t, what):
    if not torch.is_tensor(t):
        raise DudfError(f"chamfer_distance: {what} must be a tensor; got {type(t).__name__}")
    if t.device.type != "cuda":
        raise DudfError(f"chamfer_distance: {what} must live on the GPU (got {t.device}); there is no CPU fallback")
    if t.dim() == 2:
        t = t[None]
    if t.dim() != 3 or t.shape[2] != 3:
        raise DudfError(f"chamfer_distance: {what} must have shape (N, P, 3) or (P, 3); got {tuple(t.shape)}")
    return t.float()


def chamfer_distance(x, y, x_normals=None, y_normals=None, norm=2):
    """`pytorch3d.loss.chamfer_distance(x, y, x_normals=, y_normals=, norm=)` with its default reductions (point and batch
    reduction "mean", both directions, `abs_cosine=True`): returns (cham_dist, cham_normals), 0-dim float32 tensors on the input
    device; cham_normals is None without normals.  Per batch element  cham_dist = sum_x d(x, y) / P1 + sum_y d(y, x) / P2  with
    d the squared Euclidean (norm 2) or L1 (norm 1) distance to the nearest point, cham_normals the same sum of the two
    directions' means of 1 - |cos(normal, normal of the nearest point)|; both averaged over the batch.
    x, y: (N, P, 3) or (P, 3).  The other pytorch3d keywords (lengths, weights, reductions, single_directional, ...) are not
    accepted."""
    if norm not in (1, 2):
        raise ValueError("Support for 1 or 2 norm.")
    x, y = _batched(x, "x"), _batched(y, "y")
    if x.shape[0] != y.shape[0]:
        raise ValueError("x and y must have the same batch size")
    if (x_normals is None) != (y_normals is None):
        raise ValueError("x_normals and y_normals must be given together")
    have_n = x_normals is not None
    if have_n:
        x_normals, y_normals = _batched(x_normals, "x_normals"), _batched(y_normals, "y_normals")
        if x_normals.shape != x.shape or y_normals.shape != y.shape:
            raise ValueError("normals must have the shape of their points")
    N, P1, P2 = x.shape[0], x.shape[1], y.shape[1]
    if N == 0 or P1 == 0 or P2 == 0:
        raise ValueError("chamfer_distance: empty point set")
    sums = torch.zeros(N, 2, 2, dtype=torch.float64, device=x.device)           # [batch][direction][distance, normal term]
    for b in range(N):
        for d, (p, q, pn, qn) in enumerate(((x[b], y[b], x_normals[b] if have_n else None, y_normals[b] if have_n else None),
                                            (y[b], x[b], y_normals[b] if have_n else None, x_normals[b] if have_n else None))):
            dist, idx = hip_ops.nearest_points(p, q, norm, want_idx=have_n)
            hip_ops.chamfer_terms(dist, idx, pn, qn, out=sums[b, d])
    means = sums / torch.tensor([P1, P2], dtype=torch.float64, device=x.device)[None, :, None]
    per_batch = means.sum(dim=1)                                                 # (N, 2): x -> y plus y -> x
    out = per_batch.mean(dim=0).float()
    return out[0], (out[1] if have_n else None)


def vertex_normals(vertices, faces):
    """(V,3) float32 CUDA tensor: area-weighted unit vertex normals (open3d `compute_vertex_normals(normalized=True)`).
    vertices (V,3), faces (F,3): CUDA tensors."""
    return hip_ops.vertex_normals(vertices, faces)


def _cuda(a, dtype, device):
    if torch.is_tensor(a):
        if a.device.type != "cuda":
            raise DudfError(f"MeshIndex: tensors must live on the GPU (got {a.device}); there is no CPU fallback")
        return a.to(dtype)
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)      # numpy from the mesh readers


class MeshIndex:
    """The scene of a triangle mesh, built once: `MeshIndex(vertices (V,3), faces (F,3))` or `MeshIndex.from_soup(tri (T,9))`.
    Tensors are CUDA tensors; numpy arrays (what `diffudf_amd.mesh.load_obj` returns) are uploaded to `device`.  A NaN or infinite
    vertex raises ValueError."""

    def __init__(self, vertices, faces, device="cuda:0"):
        v = _cuda(vertices, torch.float32, device)
        f = _cuda(faces, torch.int64, v.device if torch.is_tensor(vertices) else device)
        if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3:
            raise DudfError(f"MeshIndex: vertices (V,3) and faces (F,3) expected; got {tuple(v.shape)}, {tuple(f.shape)}")
        if f.numel() and (int(f.min()) < 0 or int(f.max()) >= v.shape[0]):
            raise ValueError("MeshIndex: a face refers to a vertex that does not exist")
        self._init_soup(v[f].reshape(-1, 9))                       # the layout of diffudf_amd.mesh.triangle_soup

    @classmethod
    def from_soup(cls, tri, device="cuda:0"):
        self = cls.__new__(cls)
        self._init_soup(_cuda(tri, torch.float32, device))
        return self

    def _init_soup(self, tri):
        self.tri = tri.contiguous()
        self.index = hip_ops.mesh_index_build(self.tri)

    def distance(self, points, return_index=False, return_closest=False, brute=False, stats=None):
        """Unsigned distance (Q,) float32 of points (Q,3) — `scene.compute_distance(points)`; with return_index / return_closest a
        tuple (dist[, idx (Q,) int64][, closest (Q,3) float32]).  brute=True scans every triangle without the index (the same
        bits); stats: see `hip_ops.mesh_distance`."""
        dist, idx, closest = hip_ops.mesh_distance(self.tri, None if brute else self.index, points, return_index, return_closest, stats)
        if not (return_index or return_closest):
            return dist
        return (dist,) + ((idx,) if return_index else ()) + ((closest,) if return_closest else ())

    def occupancy(self, points, return_count=False, brute=False):
        """`scene.compute_occupancy(points)`: inside (Q,) bool of points (Q,3) — the parity of the triangles a ray along +x crosses
        (exact on shared edges and vertices: every crossing is counted by exactly one of the triangles that meet there); with
        return_count (inside, count (Q,) int32).  An open mesh has a parity too, it just is not an inside.  A NaN point: False,
        count -1.  brute=True scans every triangle without the index (the same counts)."""
        count, inside = hip_ops.mesh_occupancy(self.tri, None if brute else self.index, points)
        inside = inside.view(torch.bool)
        return (inside, count) if return_count else inside

    def signed_distance(self, points):
        """`scene.compute_signed_distance(points)` (Q,) float32: `distance` with the sign of `occupancy`, negative inside (open3d's
        convention); the magnitude is `distance` bit for bit, a NaN point gives NaN."""
        dist = self.distance(points)
        return torch.where(self.occupancy(points), -dist, dist)

    def trace_rays(self, rays, t0, mask, surface_eps=0.001, max_iterations=30, bound=1.3, brute=False):
        """The sphere-tracing loop of reference src/render_st.py:255-268 against this mesh in ONE launch: rays (m,3) and t0 (m,3)
        float64 CUDA tensors, mask (m,) uint8; per iteration t0 of the live rays advances by its `distance`, a ray hits when that is
        below surface_eps and dies outside (-bound, bound)^3.  t0 and mask are updated in place; returns hits (m,) uint8."""
        return hip_ops.mesh_trace_rays(self.tri, None if brute else self.index, rays, t0, mask, surface_eps, max_iterations, bound)


def mesh_distance(points, vertices, faces):
    """One-shot `MeshIndex(vertices, faces).distance(points)`."""
    dev = points.device if torch.is_tensor(points) and points.device.type == "cuda" else "cuda:0"
    return MeshIndex(vertices, faces, device=dev).distance(points)


# ---- surface-sampled evaluation (csrc/dudf_surfsample.hip) ---------------------------------------------------------
def _mesh_tensors(vertices, faces, device="cuda:0"):
    """(vertices (V,3) float64, faces (F,3) int64) on the device: CUDA tensors as they are, numpy arrays uploaded as MeshIndex does."""
    v = _cuda(vertices, torch.float64, device)
    f = _cuda(faces, torch.int64, v.device)
    if f.numel() == 0:
        f = f.reshape(0, 3)
    if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3:
        raise DudfError(f"vertices (V,3) and faces (F,3) expected; got {tuple(v.shape)}, {tuple(f.shape)}")
    return v, f


def sample_surface(vertices, faces, n, seed=123, start=0, return_face=False, uniforms=None):
    """(points (n,3) float32, normals (n,3) float32[, face (n,) int64]): area-uniform samples of a triangle mesh with the normal of
    the face each falls on, on the device.  Sample i has the global index start + i and is a pure function of (mesh, seed, start + i):
    `sample_surface(v, f, a + b)` is `sample_surface(v, f, a)` followed by `sample_surface(v, f, b, start=a)`, bit for bit.  Faces
    are chosen by integer weights floor(|e1 x e2| / max * 2^32); a degenerate face is never chosen.  uniforms (n,3)
    float64: the three numbers (face, r1, r2) of every sample instead of the generator's; an entry outside [0, 1) raises ValueError.
    Inputs are CUDA tensors, or numpy arrays (uploaded to cuda:0)."""
    v, f = _mesh_tensors(vertices, faces)
    if uniforms is not None:
        uniforms = _cuda(uniforms, torch.float64, v.device).contiguous()
        if uniforms.numel() and not bool(((uniforms >= 0.0) & (uniforms < 1.0)).all()):
            raise ValueError("sample_surface: uniforms must lie in [0, 1)")
    points, normals, face, _, _ = hip_ops.mesh_sample_surface(v, f, n, seed=seed, start=start, uniforms=uniforms, want_face=return_face)
    return (points, normals, face) if return_face else (points, normals)


def face_normals(vertices, faces):
    """(F,3) float32: (b - a) x (c - a) / max(|.|, 1e-300) of every face, formed in fp64 — `mesh.triangle_normals_areas` on the device."""
    v, f = _mesh_tensors(vertices, faces)
    return hip_ops.mesh_sample_surface(v, f, 0, want_points=False, want_normals=False, want_face_normals=True)[3]


def surface_area(vertices, faces):
    """The area of the mesh, a float: half the sum of |e1 x e2| in fp64 (a fixed order of additions)."""
    v, f = _mesh_tensors(vertices, faces)
    return float(hip_ops.mesh_sample_surface(v, f, 0, want_points=False, want_normals=False, want_area=True)[4].item())


def _stats_dict(counts, mx, sums, K):
    c, s = counts.tolist(), sums.tolist()
    return {"count_le": c[:K], "nan": c[K], "max": float(mx.item()), "sum": s[0], "sum_sq": s[1]}


def distance_stats(dist, thresholds=()):
    """dict(count_le, nan, max, mean, mean_sq) of a distance vector (n,) float32 on the device: count_le[k] = rows with
    d <= thresholds[k] (inclusive, compared in double), nan = NaN rows (left out of everything else; +inf is a value), max, and the
    means of d and d*d over the rows that are not NaN (NaN when there is none).  At most 16 thresholds."""
    dist = hip_ops._tensor(dist, "distance_stats: dist", torch.float32, (), convert=True)
    K = len(thresholds)
    st = _stats_dict(*hip_ops.distance_stats(dist, thresholds), K)
    valid = dist.shape[0] - st["nan"]
    return {"count_le": st["count_le"], "nan": st["nan"], "max": st["max"],
            "mean": st["sum"] / valid if valid else float("nan"), "mean_sq": st["sum_sq"] / valid if valid else float("nan")}


def fscore(precision, recall):
    """2 P R / (P + R), and 0 when P + R = 0."""
    return 2.0 * precision * recall / (precision + recall) if precision + recall > 0 else 0.0


def surface_metrics(vertices, faces, gt_points, gt_normals=None, gt_mesh=None, n_samples=100000, taus=(0.005, 0.01), seed=123,
                    point_to_surface=True):
    """Surface-sampled evaluation of a reconstructed mesh (vertices, faces) against a ground truth, the protocol of CAP-UDF, MeshUDF
    and NDF: a dict of floats.  The ground truth is the cloud gt_points (n,3) with gt_normals (or None), and / or the mesh
    gt_mesh = (vertices, faces); at least one of them.  All distances are Euclidean (not squared).

    Accuracy direction (reconstruction -> ground truth): `n_samples` area-uniform samples of the reconstruction (`sample_surface`
    with `seed`); the distance of each to gt_mesh (`MeshIndex.distance`, exact) when it is given, else to its nearest row of
    gt_points (`nearest_points`).
    Completeness direction (ground truth -> reconstruction): the rows of gt_points, or `n_samples` samples of gt_mesh when no cloud
    is given; the exact distance of each to the reconstructed surface (`MeshIndex.distance`), or with point_to_surface=False the
    distance to the nearest of the accuracy direction's samples — the sample-to-sample protocol of the other papers.

      accuracy, completeness    the mean distance of each direction (NaN rows left out)
      chamfer_l1                (accuracy + completeness) / 2
      chamfer_l2                the same over squared distances
      hausdorff                 the larger of the two maxima
      precision[tau]            share of the accuracy direction's rows (NaN rows left out) with distance <= tau
      recall[tau]               the same of the completeness direction
      fscore[tau]               2 P R / (P + R), 0 when P + R = 0
      normal_consistency        mean of the two directions' mean |cos| between the face normal of the sample (or of the closest
                                triangle of the reconstruction) and the matched ground-truth normal (the closest triangle's, or the
                                nearest cloud point's); None unless both directions have ground-truth normals
      n_samples, area           the sample count and the area of the reconstruction

    precision, recall and fscore are dicts keyed by the taus as given.  Everything runs on the device; the scalars are read at the end."""
    taus = tuple(taus)
    n_samples = int(n_samples)
    if n_samples <= 0:
        raise ValueError("surface_metrics: n_samples must be positive")
    if gt_points is None and gt_mesh is None:
        raise ValueError("surface_metrics: give gt_points, gt_mesh or both")
    v, f = _mesh_tensors(vertices, faces)
    dev = v.device
    samples, s_normals, _, rec_fn, area = hip_ops.mesh_sample_surface(v, f, n_samples, seed=seed, want_face_normals=True, want_area=True)
    gt_fn = gt_index = None
    if gt_mesh is not None:
        gv, gf = _mesh_tensors(gt_mesh[0], gt_mesh[1], dev)
        gt_index = MeshIndex(gv, gf)
    if gt_points is not None:
        gt = _cuda(gt_points, torch.float32, dev).contiguous()
        gt_n = None if gt_normals is None else _cuda(gt_normals, torch.float32, dev).contiguous()
        if gt_mesh is not None:
            gt_fn = face_normals(gv, gf)
    else:
        gt, gt_n, _, gt_fn, _ = hip_ops.mesh_sample_surface(gv, gf, n_samples, seed=seed, want_face_normals=True)

    cos_terms = []               # per direction with normals on both sides: (`chamfer_terms` sums, rows); mean |cos| = 1 - sums[1] / rows
    # accuracy: the reconstruction's samples against the ground truth
    if gt_index is not None:
        d_acc, i_acc = gt_index.distance(samples, return_index=True)
        acc_other = gt_fn
    else:
        d2, i_acc = hip_ops.nearest_points(samples, gt, 2)
        d_acc = torch.sqrt(d2)
        acc_other = gt_n
    acc = hip_ops.distance_stats(d_acc, taus)
    if acc_other is not None:
        cos_terms.append((hip_ops.chamfer_terms(d_acc, i_acc, s_normals, acc_other), d_acc.shape[0]))
    # completeness: the ground truth against the reconstruction
    if point_to_surface:
        d_comp, i_comp = MeshIndex(v, f).distance(gt, return_index=True)
        comp_other = rec_fn
    else:
        d2, i_comp = hip_ops.nearest_points(gt, samples, 2)
        d_comp = torch.sqrt(d2)
        comp_other = s_normals
    comp = hip_ops.distance_stats(d_comp, taus)
    if gt_n is not None:
        cos_terms.append((hip_ops.chamfer_terms(d_comp, i_comp, gt_n, comp_other), d_comp.shape[0]))

    # the scalars leave the device here
    K = len(taus)
    a, c = _stats_dict(*acc, K), _stats_dict(*comp, K)
    na, nc = d_acc.shape[0] - a["nan"], d_comp.shape[0] - c["nan"]
    mean = lambda s, m: s / m if m else float("nan")     # noqa: E731
    out = {"accuracy": mean(a["sum"], na), "completeness": mean(c["sum"], nc)}
    out["chamfer_l1"] = 0.5 * (out["accuracy"] + out["completeness"])
    out["chamfer_l2"] = 0.5 * (mean(a["sum_sq"], na) + mean(c["sum_sq"], nc))
    out["hausdorff"] = max(a["max"], c["max"])
    out["precision"] = {t: mean(a["count_le"][k], na) for k, t in enumerate(taus)}
    out["recall"] = {t: mean(c["count_le"][k], nc) for k, t in enumerate(taus)}
    out["fscore"] = {t: fscore(out["precision"][t], out["recall"][t]) if na and nc else float("nan") for t in taus}
    out["normal_consistency"] = (0.5 * sum(1.0 - float(s[1].item()) / m for s, m in cos_terms)) if len(cos_terms) == 2 else None
    out["n_samples"] = n_samples
    out["area"] = float(area.item())
    return out
