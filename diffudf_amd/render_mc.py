# coding: utf-8
"""Field extraction and CAP-UDF meshing for the marching-cubes consumers — reference src/render_mc.py:20-99
`extract_fields` and :201-256 `extract_mesh_CAP` (BASELINE config 5: the batched field+gradient query feeding CAP-UDF
extraction, all on the device) — and :101-199 `extract_mesh_MESHUDF`, the MeshUDF marching cubes over the same fields, on
the host (C++ library behind `marching_cubes.udf_mc_lewiner`; serial by nature) — and :259-406, the
signed path of gt_mode 'siren': `gen_sdf_coordinate_grid`, `get_mesh_sdf` (raw network values on the grid, then Lewiner's marching
cubes, both on the device) and `convert_sdf_samples_to_ply`."""
import numpy as np
import torch

from . import hip_ops
from ._lib import DudfError


def _eigenvector_fallback(cfg, theta, N, vec, rows, idx):
    """The rare path of `extract_fields` (reference :77-93) for both field layouts: rows `rows` of `vec` (P, 3), which are the grid
    points of linear index `idx` (first axis slowest), are recomputed with the Hessian frame — the top eigenvector, sign-aligned
    with what the epilogue left there."""
    voxel = 2.0 / (N - 1)
    xyz = torch.stack([(idx // (N * N)) % N, (idx // N) % N, idx % N], 1).float() * voxel - 1.0
    _, _, _, _, V = hip_ops.query_frame(cfg, theta, xyz)
    n_hat = V[:, :, 2]
    sign = torch.where((vec[rows] * n_hat).sum(-1, keepdim=True) < 0, -1.0, 1.0)
    vec[rows] = sign * n_hat


def extract_fields(decoder, latent_vec, N, gt_mode, device, alpha, chunk=1 << 20):
    """Same signature and return contract as the reference: (df_values (N,N,N), vecs (N,N,N,3)) float32 tensors on
    `device`.  df = inverse(gt_mode, |f|, alpha); vecs = -normalize(grad f), or the top Hessian eigenvector aligned with
    it where the normalised gradient is shorter than 0.04 (a vanishing gradient).

    Unlike the reference (3 float64 numpy arrays of N^3 rows and 4096-point chunks through PyTorch autograd, with
    the Hessian evaluated for EVERY grid point), coordinates are derived from the grid index inside the kernel,
    value and gradient come from the fused sweeps in 2^20-point chunks, the inverse map / normalisation are a kernel
    epilogue, and the Hessian path runs only for the points that take the fallback (normally none)."""
    if latent_vec is not None and torch.as_tensor(latent_vec).numel() != 0:
        raise DudfError("extract_fields: latent vectors are not part of the HIP path")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise DudfError("extract_fields: needs the GPU; there is no CPU fallback path")
    cfg = decoder.hip_cfg
    theta = decoder.flat_parameters()
    total = N ** 3
    df = torch.empty(total, dtype=torch.float32, device=dev)
    vec = torch.empty(total, 3, dtype=torch.float32, device=dev)
    flags = []
    start = 0
    ws = hip_ops.query_workspace_for(cfg, min(chunk, total), dev)
    while start < total:
        cnt = min(chunk, total - start)
        w = ws if cnt == ws.n else hip_ops.QueryWorkspace(cfg, cnt, dev)
        flags.append((start, cnt, hip_ops.grid_fields(cfg, theta, N, start, cnt, gt_mode, alpha, df, vec, w)))
        start += cnt
    if int(torch.stack([f for _, _, f in flags]).sum()) > 0:
        bad = (vec.norm(dim=-1) < 0.04).nonzero().flatten()
        _eigenvector_fallback(cfg, theta, N, vec, bad, bad.to(torch.int64))
    return df.reshape(N, N, N), vec.reshape(N, N, N, 3)


class TriangleSoup:
    """What `extract_mesh_CAP` returns when `trimesh` is not installed: the two arrays a `trimesh.Trimesh(v, f,
    process=False)` would hold, plus OBJ / PLY export (the reference only ever calls `.export(path)` and reads
    `.vertices` / `.faces`, generate_mc.py:60-75)."""

    def __init__(self, vertices, faces, vertex_normals=None):
        self.vertices = np.asarray(vertices, dtype=np.float64)
        self.faces = np.asarray(faces, dtype=np.int64)
        self._vertex_normals = None if vertex_normals is None else np.asarray(vertex_normals, dtype=np.float64)

    @property
    def vertex_normals(self):
        """(V,3) float64 area-weighted unit vertex normals (what `mesh.as_open3d.compute_vertex_normals(normalized=True)` gives the
        reference's cuantitative.py:99-100), computed on the device by `metrics.vertex_normals`."""
        if self._vertex_normals is not None:           # given by the extraction (`get_mesh_sdf`), as trimesh keeps them
            return self._vertex_normals
        from . import metrics
        dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        n = metrics.vertex_normals(torch.from_numpy(np.ascontiguousarray(self.vertices)).to(dev),
                                   torch.from_numpy(np.ascontiguousarray(self.faces)).to(dev))
        return n.cpu().numpy().astype(np.float64)

    def export(self, path):
        v, f = self.vertices, self.faces
        if str(path).endswith(".ply"):
            with open(path, "w") as fo:
                fo.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty double x\nproperty double y\nproperty double z\n"
                         "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(v), len(f)))
                np.savetxt(fo, v, fmt="%.17g")
                np.savetxt(fo, np.concatenate([np.full((len(f), 1), 3), f], 1), fmt="%d")
        else:
            with open(path, "w") as fo:
                np.savetxt(fo, v, fmt="v %.17g %.17g %.17g")
                np.savetxt(fo, f + 1, fmt="f %d %d %d")
        return path


_FINISH_KEYS = ("min_faces", "min_area", "min_area_ratio", "keep_largest", "simplify")


_SIMPLIFY_KEYS = ("grid", "cell", "target_faces", "boundary_weight", "origin")


def _finish_soup(v, f, finish):
    """The per-cell soup (device tensors) as a mesh, on the device: welded and pruned (`meshclean.clean_mesh(fill_holes=False)`),
    wound consistently per component (`meshclean.orient_faces`; CAP-UDF signs each cell on its own, so neighbouring cells disagree
    on about one shared edge in six), and with a dict of `meshclean.remove_small_components` keywords the floaters dropped.  The dict
    key "simplify" holds a dict of `meshclean.simplify_mesh` keywords (grid / cell / target_faces, boundary_weight, origin): the mesh is
    then clustered last, behind welding, winding and the component filter, and wound again (orient=True)."""
    if finish != "mesh" and not (isinstance(finish, dict) and all(k in _FINISH_KEYS for k in finish)):
        raise ValueError(f"finish must be None, 'mesh' or a dict over {_FINISH_KEYS}; got {finish!r}")
    simplify = finish.get("simplify") if isinstance(finish, dict) else None
    if simplify is not None and not (isinstance(simplify, dict) and all(k in _SIMPLIFY_KEYS for k in simplify)):
        raise ValueError(f"finish['simplify'] must be a dict over {_SIMPLIFY_KEYS}; got {simplify!r}")
    from . import meshclean
    v, f, _ = meshclean.clean_mesh(v, f, fill_holes=False)
    if isinstance(finish, dict):
        v, f, _ = meshclean.remove_small_components(v, f, **{k: x for k, x in finish.items() if k != "simplify"})
    else:
        f = meshclean.orient_faces(v, f)
    if simplify is not None:
        v, f, _ = meshclean.simplify_mesh(v, f, orient=True, **simplify)
    return v, f


def extract_mesh_CAP(ndf, grad, resolution, threshold=0.008, device=None, finish=None):
    """Same signature as reference src/render_mc.py:201 (`ndf` (N,N,N), `grad` (N,N,N,3): numpy arrays or tensors — the
    outputs of `extract_fields` can be passed straight through without leaving the device).  Active-cell test, sign by
    gradient, per-cell marching cubes and compaction run in `dudf_capudf_count` / `dudf_capudf_emit`; returns a
    `trimesh.Trimesh(process=False)` when trimesh is importable, else a `TriangleSoup` with the same two arrays.
    `finish`: None — the per-cell triangle soup (no vertex is shared between cells), as the reference; "mesh" — welded and consistently wound on the device
    (`_finish_soup`); a dict over min_faces / min_area / min_area_ratio / keep_largest — the same, then the small components
    dropped (`meshclean.remove_small_components`); its key "simplify": a dict of `meshclean.simplify_mesh` keywords, applied last."""
    dev = torch.device(device) if device is not None else (ndf.device if torch.is_tensor(ndf) and ndf.is_cuda else torch.device("cuda", 0))
    if dev.type != "cuda":
        raise DudfError("extract_mesh_CAP: needs the GPU; there is no CPU fallback path")
    t = lambda a: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(dev)   # noqa: E731
    d, g = t(ndf), t(grad)
    if d.shape[0] != resolution:
        raise ValueError("resolution does not match the field")
    v, f = hip_ops.capudf_extract(d, g, threshold)
    if finish is not None:
        v, f = _finish_soup(v, f, finish)
    return _as_mesh(v.cpu().numpy(), f.cpu().numpy())


def _as_mesh(v, f):
    try:
        import trimesh
        return trimesh.Trimesh(v, f, process=False)
    except ImportError:
        return TriangleSoup(v, f)


class SparseFields:
    """The fields of `extract_fields` on a brick-sparse narrow band (layout: include/dudf_hip.h).

    N, brick, threshold, lipschitz : what the bricks were selected for;
    slot (nl,nl,nl) int32          : slot of a stored brick or -1, nl = (N-1) // brick + 1, slots in ascending brick id;
    stored_ids, candidate_ids      : ascending int32 brick ids ((b0 * nl + b1) * nl + b2) of the stored bricks (slot order) and of
                                     the candidate bricks, the ones whose cells are walked;
    df (S,B,B,B), vec (S,B,B,B,3)  : float32 fields of the stored bricks; a point beyond the grid in a partial brick holds the
                                     value at the clamped index and is never read.
    All device tensors.  `to_dense` / `from_dense` are a gather and a scatter with torch indexing, for tests and debugging."""

    def __init__(self, N, brick, threshold, lipschitz, slot, stored_ids, candidate_ids, df, vec):
        self.N, self.brick, self.threshold, self.lipschitz = int(N), int(brick), float(threshold), float(lipschitz)
        self.slot, self.stored_ids, self.candidate_ids, self.df, self.vec = slot, stored_ids, candidate_ids, df, vec

    @property
    def points_stored(self):
        return int(self.stored_ids.numel()) * self.brick ** 3

    def grid_index(self):
        """(lin, valid), both (S,B,B,B): the linear grid index (first axis slowest, clamped to the grid) of every stored point and
        whether the point lies in the grid (False: padding of a partial brick)."""
        return _brick_grid_index(self.stored_ids, self.N, self.brick)

    def to_dense(self, fill=float("nan")):
        """(ndf (N,N,N), vec (N,N,N,3)) with `fill` wherever nothing is stored."""
        N = self.N
        lin, valid = self.grid_index()
        ndf = torch.full((N ** 3,), fill, dtype=torch.float32, device=self.df.device)
        vec = torch.full((N ** 3, 3), fill, dtype=torch.float32, device=self.df.device)
        ndf[lin[valid]] = self.df[valid]
        vec[lin[valid]] = self.vec[valid]
        return ndf.reshape(N, N, N), vec.reshape(N, N, N, 3)

    @classmethod
    def from_dense(cls, ndf, vec, threshold=0.008, brick=8, lipschitz=1.25):
        """The bricks `dudf_sparse_select` keeps for the dense device fields ndf (N,N,N), vec (N,N,N,3), filled from them."""
        ndf = hip_ops._tensor(ndf, "ndf", torch.float32, convert=True)
        vec = hip_ops._tensor(vec, "vec", torch.float32, convert=True)
        N = ndf.shape[0]
        if ndf.shape != (N, N, N) or vec.shape != (N, N, N, 3):
            raise DudfError(f"SparseFields.from_dense: ndf (N,N,N) and vec (N,N,N,3) expected, got {tuple(ndf.shape)}, {tuple(vec.shape)}")
        m, nb, nl = hip_ops.sparse_dims(N, brick)
        at = torch.clamp(torch.arange(nb + 1, device=ndf.device) * brick, max=m)
        coarse = ndf[at][:, at][:, :, at].contiguous()
        slot, stored, cands = hip_ops.sparse_select(coarse, N, brick, hip_ops.sparse_bound(N, brick, threshold, lipschitz))
        lin, _ = _brick_grid_index(stored, N, brick)
        return cls(N, brick, threshold, lipschitz, slot, stored, cands, ndf.reshape(-1)[lin].contiguous(),
                   vec.reshape(-1, 3)[lin].contiguous())

    def extract(self, threshold=None, want_cells=False, want_counts=False):
        """`hip_ops.capudf_sparse_extract` on these fields (device tensors); `threshold` at most the one they were selected for."""
        thr = self.threshold if threshold is None else float(threshold)
        if thr > self.threshold:
            raise ValueError(f"threshold {thr} exceeds the {self.threshold} these bricks were selected for: cells could be missed")
        return hip_ops.capudf_sparse_extract(self.df, self.vec, self.slot, self.candidate_ids, self.N, self.brick, thr,
                                             want_cells=want_cells, want_counts=want_counts)


def _brick_grid_index(stored_ids, N, brick):
    m, nb, nl = hip_ops.sparse_dims(N, brick)
    ids = stored_ids.to(torch.int64)
    loc = torch.arange(brick, device=ids.device)
    g = [(b * brick)[:, None] + loc for b in (ids // (nl * nl), (ids // nl) % nl, ids % nl)]               # (S, B) per axis
    g0, g1, g2 = g[0][:, :, None, None], g[1][:, None, :, None], g[2][:, None, None, :]
    valid = (g0 <= m) & (g1 <= m) & (g2 <= m)
    lin = (g0.clamp(max=m) * N + g1.clamp(max=m)) * N + g2.clamp(max=m)
    return lin, valid


def extract_fields_sparse(decoder, latent_vec, N, gt_mode, device, alpha, threshold=0.008, brick=8, lipschitz=1.25, chunk=1 << 20):
    """`extract_fields` on a narrow band: the network is evaluated on a coarse lattice (every `brick`-th grid point, value only),
    the bricks that can hold a cell with a corner value <= `threshold` are selected, and the fine grid is evaluated inside those
    only.  Returns a `SparseFields`; `extract_mesh_CAP_sparse` meshes it.  A stored point has the coordinates,
    and therefore the chunk-independent values, of the dense grid.

    The selection keeps a cell brick when a corner of it has df <= threshold + lipschitz * (half the brick's diagonal).  That covers
    every active cell IF df changes by at most `lipschitz` per unit length.  `lipschitz` is the caller's statement about their field:
    a distance field has 1, the default 1.25 leaves a learned one a quarter of slack, and nothing here can verify it — where a
    learned field is steeper than that between lattice points, cells can be missed.  The dense path stays the exact one
    (`tools/bench_sparse_mc.py` reports the difference of the two emitted-cell sets for a checkpoint).

    Memory: 16 bytes per stored point, plus the sweeps' workspace of one chunk — about 16 KB per point of `chunk` for an 8x256
    network, 16 GB at the default 2^20, which `extract_fields` allocates too; `chunk=1 << 16` brings it to 1 GB."""
    if latent_vec is not None and torch.as_tensor(latent_vec).numel() != 0:
        raise DudfError("extract_fields_sparse: latent vectors are not part of the HIP path")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise DudfError("extract_fields_sparse: needs the GPU; there is no CPU fallback path")
    m, nb, nl = hip_ops.sparse_dims(N, brick)
    cfg = decoder.hip_cfg
    theta = decoder.flat_parameters()
    B3 = brick ** 3

    def chunks(total, step):                               # one workspace, sized for a whole chunk, serves the shorter last call too
        if total == 0:
            return
        ws = hip_ops.query_workspace_for(cfg, min(step, total), dev)
        for start in range(0, total, step):
            yield start, min(step, total - start), ws

    coarse = torch.empty((nb + 1) ** 3, dtype=torch.float32, device=dev)
    for start, cnt, w in chunks(coarse.numel(), chunk):
        hip_ops.grid_fields_lattice(cfg, theta, N, brick, start, cnt, gt_mode, alpha, coarse, None, w)
    slot, stored, cands = hip_ops.sparse_select(coarse, N, brick, hip_ops.sparse_bound(N, brick, threshold, lipschitz))
    del coarse
    S = int(stored.numel())
    if S * B3 > 2 ** 31 - 1:
        raise DudfError(f"extract_fields_sparse: {S} bricks of {B3} points exceed 2^31 - 1 stored points; lower N, threshold or lipschitz")
    df = torch.empty(S, brick, brick, brick, dtype=torch.float32, device=dev)
    vec = torch.empty(S, brick, brick, brick, 3, dtype=torch.float32, device=dev)
    per = max(1, chunk // B3)                              # bricks per call
    flags = [hip_ops.grid_fields_bricks(cfg, theta, N, brick, stored, s // B3, c // B3, gt_mode, alpha, df, vec, w)
             for s, c, w in chunks(S * B3, per * B3)]
    if flags and int(torch.stack(flags).sum()) > 0:
        flat = vec.view(-1, 3)
        bad = (flat.norm(dim=-1) < 0.04).nonzero().flatten()
        lin, _ = _brick_grid_index(stored, N, brick)
        _eigenvector_fallback(cfg, theta, N, flat, bad, lin.reshape(-1)[bad])
    return SparseFields(N, brick, threshold, lipschitz, slot, stored, cands, df, vec)


def extract_mesh_CAP_sparse(fields, threshold=None, finish=None):
    """`extract_mesh_CAP` on the `SparseFields` of `extract_fields_sparse`: the same per-cell code (`dudf_capudf_sparse_count` /
    `_emit`) over the cells of the candidate bricks, so wherever both paths walk a cell they emit the same triangles bit for bit.
    `threshold` defaults to the one the fields were selected for and may not exceed it (ValueError).  Returns a
    `trimesh.Trimesh(process=False)` when trimesh is importable, else a `TriangleSoup`.  `finish`: as `extract_mesh_CAP`."""
    v, f = fields.extract(threshold)
    if finish is not None:
        v, f = _finish_soup(v, f, finish)
    return _as_mesh(v.cpu().numpy(), f.cpu().numpy())


def extract_mesh_MESHUDF(df_values, normals, device, smooth_borders=False, luts=None, clean=None, **kwargs):
    """Reference src/render_mc.py:101-199 (`extract_mesh_MESHUDF`): the MeshUDF marching cubes over the (N, N, N) field and
    its (N, N, N, 3) direction field (outputs of `extract_fields`; tensors or numpy arrays), vertices shifted to
    [-1, 1]^3.  The extraction itself — the reference's Cython extension — is `diffudf_amd.marching_cubes.udf_mc_lewiner`
    over the host C++ library (bit-identical vertices and faces, tests/test_meshudf.py); the Lewiner tables come from the
    caller (`luts=`: a dict or a path) or from `marching_cubes.load_luts()` ($DUDF_MESHUDF_LUTS, then the reference's own
    `_marching_cubes_lewiner_luts.py` on `sys.path`); none found: MeshUDFError.  Tensors come back on `device`, as in
    the reference.
    Returns (vertices, faces, mesh).  The reference then cleans the mesh with trimesh (`process`, duplicate / degenerate
    faces, `fill_holes`, optional Laplacian smoothing of the border).  `clean`:
      None      trimesh exactly as the reference when it is importable; otherwise the device clean-up (`meshclean.clean_mesh`,
                then `meshclean.smooth_borders` when `smooth_borders`) when `device` is a CUDA device; otherwise (a CPU device
                without trimesh) the raw extraction, `smooth_borders` ignored;
      "device"  the device clean-up whether or not trimesh is there; a CPU device: DudfError;
      False     the raw extraction.
    Without trimesh the mesh is a `TriangleSoup` of what is returned."""
    if clean not in (None, False, "device"):
        raise ValueError(f"clean must be None, False or 'device'; got {clean!r}")
    if clean == "device" and torch.device(device).type != "cuda":
        raise DudfError("extract_mesh_MESHUDF(clean='device'): needs the GPU; there is no CPU fallback path")
    from .marching_cubes import udf_mc_lewiner
    d = df_values.detach().cpu().numpy() if torch.is_tensor(df_values) else np.asarray(df_values)
    g = normals.detach().cpu().numpy() if torch.is_tensor(normals) else np.asarray(normals)
    d = np.where(d < 0, 0, d).astype(np.float32)
    N = d.shape[0]
    voxel_size = 2.0 / (N - 1)
    verts, faces, _, _ = udf_mc_lewiner(d, g.astype(np.float32), spacing=[voxel_size] * 3, avg_thresh=1.05, max_thresh=1.75, luts=luts)
    verts = verts - 1                                   # voxel origin (-1, -1, -1)
    if len(faces) == 0:
        raise ValueError("Could not find surface in volume")
    trimesh = None
    if clean is None:
        try:
            import trimesh
        except ImportError:
            pass
    if trimesh is None:
        if clean == "device" or (clean is None and torch.device(device).type == "cuda"):
            from . import meshclean
            dv, dfc, _ = meshclean.clean_mesh(verts, faces, device=device)
            if smooth_borders:
                dv = meshclean.smooth_borders(dv, dfc)
            return dv.float(), dfc, TriangleSoup(dv.cpu().numpy(), dfc.cpu().numpy())
        mesh = TriangleSoup(verts, faces)
        return (torch.from_numpy(np.ascontiguousarray(verts)).float().to(device),
                torch.from_numpy(np.ascontiguousarray(faces)).long().to(device), mesh)
    mesh = trimesh.Trimesh(verts, faces).process(validate=False)
    mesh.remove_duplicate_faces(); mesh.remove_degenerate_faces(); mesh.fill_holes()
    mesh2 = trimesh.Trimesh(mesh.vertices, mesh.faces)
    nv, nf, it = 0, 0, 0
    while (nv, nf) != (len(mesh2.vertices), len(mesh2.faces)) and it < 10:
        mesh2 = mesh2.process(validate=False)
        mesh2.remove_duplicate_faces(); mesh2.remove_degenerate_faces()
        nv, nf = len(mesh2.vertices), len(mesh2.faces)
        it += 1
        mesh2 = trimesh.Trimesh(mesh2.vertices, mesh2.faces)
    mesh = trimesh.Trimesh(mesh2.vertices, mesh2.faces)
    if smooth_borders:
        from collections import defaultdict
        from scipy.sparse import coo_matrix
        border = trimesh.grouping.group_rows(mesh.edges_sorted, require_count=1)
        nb = defaultdict(list)
        for u, v in mesh.edges_sorted[border]:
            nb[u].append(v); nb[v].append(u)
        bv = np.array(list(nb.keys()))
        if len(bv) > 0:
            pi, pj = [], []
            for k, ns in enumerate(nb.values()):
                for j in ns:
                    pi.append(k); pj.append(j)
            sp = coo_matrix((np.ones(len(pi)), (pi, pj)), shape=(len(bv), len(mesh.vertices)))
            for _ in range(5):
                avg = sp @ mesh.vertices / sp.sum(axis=1)
                mesh.vertices[bv] = mesh.vertices[bv] + 0.3 * (np.asarray(avg) - mesh.vertices[bv])
    return torch.tensor(mesh.vertices).float().to(device), torch.tensor(mesh.faces).long().to(device), mesh


def gen_sdf_coordinate_grid(N, voxel_size, device, voxel_origin=[-1, -1, -1]):
    """Reference src/render_mc.py:259-311: the (N**3, 4) float32 tensor on `device` whose first three columns are the grid
    coordinates (first axis slowest; column k = index_k * voxel_size + voxel_origin[2 - k]) and whose last column, zero, is
    where the reference stores the values.  `get_mesh_sdf` here does not need it (the kernel derives coordinates from the
    index); it is kept for callers of the reference's function."""
    overall_index = torch.arange(0, N ** 3, 1, dtype=torch.int64)
    samples = torch.zeros(N ** 3, 4, device=device, requires_grad=False)
    samples[:, 2] = overall_index % N
    samples[:, 1] = (overall_index.long() / N) % N
    samples[:, 0] = ((overall_index.long() / N) / N) % N
    samples[:, 0] = (samples[:, 0] * voxel_size) + voxel_origin[2]
    samples[:, 1] = (samples[:, 1] * voxel_size) + voxel_origin[1]
    samples[:, 2] = (samples[:, 2] * voxel_size) + voxel_origin[0]
    return samples


def sdf_grid_values(decoder, N, device, max_batch=64 ** 3):
    """The (N, N, N) float32 device tensor of raw network outputs on the grid (`dudf_grid_values` in chunks of `max_batch`)."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise DudfError("get_mesh_sdf: needs the GPU; there is no CPU fallback path")
    cfg = decoder.hip_cfg
    theta = decoder.flat_parameters()
    total = N ** 3
    out = torch.empty(total, dtype=torch.float32, device=dev)
    chunk = max(1, min(int(max_batch), total))
    ws = hip_ops.query_workspace_for(cfg, chunk, dev)
    start = 0
    while start < total:
        cnt = min(chunk, total - start)
        hip_ops.grid_values(cfg, theta, N, start, cnt, out, ws if cnt == ws.n else hip_ops.QueryWorkspace(cfg, cnt, dev))
        start += cnt
    return out.reshape(N, N, N)


def convert_sdf_samples_to_ply(pytorch_3d_sdf_tensor, voxel_grid_origin, voxel_size, offset=None, scale=None, luts=None):
    """Reference src/render_mc.py:360-406: marching cubes at level 0 of an (n, n, n) field, vertices moved to the voxel origin,
    then `/ scale` and `- offset`.  A field without the zero level prints the reference's message and gives empty arrays.  A CUDA
    tensor stays on the device (tensors come back); a CPU tensor or numpy array runs in the host library (numpy comes back)."""
    from .marching_cubes import marching_cubes_lewiner
    vol = pytorch_3d_sdf_tensor
    on_dev = torch.is_tensor(vol) and vol.is_cuda
    if torch.is_tensor(vol) and not on_dev:
        vol = vol.numpy()
    verts, faces, normals, values = np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0)
    level = 0.0
    if level < float(vol.min()) or level > float(vol.max()):
        print("Surface level must be within volume data range.")
        if on_dev:
            verts, faces, normals, values = (torch.from_numpy(a).to(vol.device) for a in (verts, faces, normals, values))
    else:
        verts, faces, normals, values = marching_cubes_lewiner(vol, level, spacing=[voxel_size] * 3, luts=luts)
    mesh_points = torch.zeros_like(verts) if on_dev else np.zeros_like(verts)
    mesh_points[:, 0] = voxel_grid_origin[0] + verts[:, 0]
    mesh_points[:, 1] = voxel_grid_origin[1] + verts[:, 1]
    mesh_points[:, 2] = voxel_grid_origin[2] + verts[:, 2]
    if on_dev:                                           # as tensors: torch divides by a Python scalar through its reciprocal
        as_dev = lambda a: torch.as_tensor(np.atleast_1d(np.asarray(a, dtype=np.float64)), device=mesh_points.device)  # noqa: E731
        scale, offset = (None if a is None else as_dev(a) for a in (scale, offset))
    if scale is not None:
        mesh_points = mesh_points / scale
    if offset is not None:
        mesh_points = mesh_points - offset
    return mesh_points, faces, normals, values


def get_mesh_sdf(decoder, N=256, device=None, max_batch=64 ** 3, offset=None, scale=None, luts=None):
    """Reference src/render_mc.py:314-358: the zero level set of a signed network on the N^3 grid of [-1, 1]^3.  The values come
    from `dudf_grid_values` in chunks of `max_batch`, the mesh from the device marching cubes; nothing of size N^3 leaves the
    device (the reference copies every chunk and the whole grid to the host and calls scikit-image).  `luts`: the Lewiner tables,
    as for `extract_mesh_MESHUDF`.  Returns (verts, faces, mesh) as numpy arrays and a `trimesh.Trimesh(vertices, faces,
    vertex_normals=normals)` when trimesh is importable, else a `TriangleSoup` that carries those normals."""
    dev = torch.device(device) if device is not None else torch.device("cuda", 0)
    if hasattr(decoder, "eval"):
        decoder.eval()
    voxel_origin = [-1, -1, -1]
    voxel_size = 2.0 / (N - 1)
    sdf_values = sdf_grid_values(decoder, N, dev, max_batch)
    verts, faces, normals, _ = convert_sdf_samples_to_ply(sdf_values, voxel_origin, voxel_size, offset, scale, luts=luts)
    verts, faces, normals = verts.cpu().numpy(), faces.cpu().numpy(), normals.cpu().numpy()
    try:
        import trimesh
        return verts, faces, trimesh.Trimesh(vertices=verts, faces=faces, vertex_normals=normals)
    except ImportError:
        return verts, faces, TriangleSoup(verts, faces, vertex_normals=normals)
