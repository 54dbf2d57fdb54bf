# coding: utf-8
"""Mesh clean-up on the device — what the reference asks of trimesh behind `extract_mesh_MESHUDF` (src/render_mc.py:136-197:
`process`, duplicate and degenerate faces, `fill_holes`, Laplacian smoothing of the border), without trimesh: weld vertices on
rint(v * 10^digits), drop degenerate, duplicate and invalid faces and unused vertices, close 3- and 4-edge holes, smooth the
border.  The rules are DESIGN.md §3 "Mesh clean-up"; the kernels are csrc/dudf_meshclean.hip.  Parity with trimesh's own vertex and
face ORDER is not pinned; the result is deterministic and equals tests/meshclean_oracle.py bit for bit.

Mesh topology (csrc/dudf_meshtopo.hip; what trimesh's `fix_winding` / `split` serve in the reference's workflows):
`face_topology`, `orient_faces`, `remove_small_components`.  The pin is tests/meshtopo_oracle.py, exactly.

Simplification (csrc/dudf_meshsimplify.hip; what trimesh / open3d decimation serve in the reference's workflows):
`simplify_mesh`, quadric vertex clustering with border quadrics.  The pin is tests/simplify_oracle.py.

Tensors stay on the device; each round reads its counts back once (they size the outputs)."""
import numpy as np
import torch

from . import hip_ops
from ._lib import DudfError


def _device_mesh(vertices, faces, device=None):
    """(vertices (V,3) float64, faces (F,3) int64) on `device`; None: the device of whichever argument is a CUDA tensor, else the
    current one."""
    t = lambda a, dt: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(dt).reshape(-1, 3)   # noqa: E731
    v, f = t(vertices, torch.float64), t(faces, torch.int64)
    if device is not None:
        dev = torch.device(device)
    else:
        dev = v.device if v.is_cuda else f.device if f.is_cuda else torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
    if dev.type != "cuda":
        raise DudfError("meshclean: needs the GPU; there is no CPU fallback path")
    return v.to(dev), f.to(dev)


def clean_mesh(vertices, faces, fill_holes=True, max_rounds=10, digits=8, device=None):
    """The reference's sequence: one round, fill the 3- and 4-edge holes, then rounds until (V, F) stops changing (at most
    `max_rounds`).  vertices (V,3), faces (F,3): tensors or numpy arrays.  Returns (vertices float64, faces int64, info) with the
    tensors on the device; info sums the rounds' counts (`hip_ops.MESH_CLEAN_COUNTS`; `vertices` and `faces` are those of the result)
    and adds `rounds`."""
    v, f = _device_mesh(vertices, faces, device)
    info, rounds = None, 0
    while True:
        n = (v.shape[0], f.shape[0])
        v, f, c = hip_ops.mesh_clean_round(v, f, digits=digits, fill_holes=bool(fill_holes) and rounds == 0)
        rounds += 1
        info = c if info is None else {k: (c[k] if k in ("vertices", "faces") else info[k] + c[k]) for k in c}
        if (rounds > 1 and (v.shape[0], f.shape[0]) == n) or rounds > max_rounds:
            break
    info["rounds"] = rounds
    return v, f, info


def border_edges(faces, n_vertices, device=None):
    """(E,2) int64 device tensor of the undirected edges that exactly one face uses, ascending."""
    _, f = _device_mesh(np.zeros((0, 3)), faces, device)
    return hip_ops.mesh_border_edges(f, n_vertices)


def smooth_borders(vertices, faces, iterations=5, lam=0.3, device=None):
    """Reference src/render_mc.py:169-197: `iterations` Jacobi steps v += lam * (mean(border neighbours) - v) on the endpoints of the
    border edges; a new (V,3) float64 device tensor."""
    v, f = _device_mesh(vertices, faces, device)
    return hip_ops.mesh_smooth_borders(v, f, iterations, lam)


AREA_UNIT = 2.0 ** -31                  # area of a component = its integer sum * AREA_UNIT (q = rint(min(nn, 16) * 2^30), area = nn / 2)


def face_topology(faces, n_vertices, vertices=None, device=None):
    """Winding, components and edge classes of a mesh.  faces (F,3), vertices None or (V,3): tensors or numpy arrays.
    Returns a dict: `faces` (F,3) int64 consistently wound, `component` (F,) int64 (the smallest face index of the face's component)
    and `flip` (F,) uint8 as device tensors; per component, on the host, `labels` (C,) int64 ascending, `n_faces` (C,) int64,
    `area_q` (C,) uint64 and `area` (C,) float64 = area_q * 2^-31 (both None without vertices); and the eight counts of
    `hip_ops.MESH_TOPOLOGY_COUNTS` by name."""
    _, f = _device_mesh(np.zeros((0, 3)), faces, device)
    v = None
    if vertices is not None:
        v, _ = _device_mesh(vertices, np.zeros((0, 3), dtype=np.int64), f.device)
    out_f, comp, flip, nfaces, area_q, counts = hip_ops.mesh_topology(f, int(n_vertices), v)
    labels = nfaces.nonzero().flatten()
    out = {"faces": out_f, "component": comp, "flip": flip, "labels": labels.cpu().numpy(), "n_faces": nfaces[labels].cpu().numpy(),
           "area_q": None, "area": None}
    if v is not None:
        out["area_q"] = area_q[labels].cpu().numpy().view(np.uint64)
        out["area"] = out["area_q"].astype(np.float64) * AREA_UNIT
    out.update(counts)
    return out


def orient_faces(vertices, faces, device=None):
    """The faces (F,3) int64 on the device, wound consistently per component: the smallest face index of a component keeps its winding
    (DESIGN.md §3.6b).  Which side is "out" is not decided here."""
    v, f = _device_mesh(vertices, faces, device)
    return hip_ops.mesh_topology(f, v.shape[0])[0]


def component_filter(labels, n_faces, area_q, min_faces=0, min_area=0.0, min_area_ratio=0.0, keep_largest=None):
    """(C,) bool: the components that stay.  One stays iff n_faces >= min_faces, area_q >= ceil(min_area * 2^31) and area_q >=
    ceil(min_area_ratio * sum(area_q)) — comparisons of integers —; keep_largest = k then keeps the k largest of those by (area_q,
    n_faces) descending, ties to the smaller label."""
    import math
    q = [int(x) for x in area_q] if area_q is not None else [0] * len(labels)
    n = [int(x) for x in n_faces]
    if area_q is None and (min_area > 0.0 or min_area_ratio > 0.0):
        raise ValueError("an area threshold needs the vertices")
    t_area = math.ceil(float(min_area) * 2147483648.0)
    t_ratio = math.ceil(float(min_area_ratio) * float(sum(q)))
    keep = [n[i] >= int(min_faces) and q[i] >= t_area and q[i] >= t_ratio for i in range(len(n))]
    if keep_largest is not None:
        order = sorted((i for i in range(len(n)) if keep[i]), key=lambda i: (-q[i], -n[i], int(labels[i])))
        keep = [False] * len(n)
        for i in order[:max(int(keep_largest), 0)]:
            keep[i] = True
    return np.array(keep, dtype=bool)


def remove_small_components(vertices, faces, min_faces=0, min_area=0.0, min_area_ratio=0.0, keep_largest=None, device=None):
    """Drop the floaters: the components `component_filter` rejects (sizes and integer areas from `face_topology`), then the submesh of
    the faces that stay (`hip_ops.mesh_submesh`: face order kept, unused vertices dropped, faces re-indexed; a face with an index
    outside [0, V) cannot be re-indexed and goes).  Returns (vertices float64, faces int64 — consistently wound —, info) on the device;
    info holds the counts of `face_topology` and `components_kept`, `components_removed`, `faces_removed`."""
    v, f = _device_mesh(vertices, faces, device)
    topo = face_topology(f, v.shape[0], v)
    keep_c = component_filter(topo["labels"], topo["n_faces"], topo["area_q"], min_faces, min_area, min_area_ratio, keep_largest)
    by_label = torch.zeros(max(f.shape[0], 1), dtype=torch.uint8, device=f.device)
    by_label[torch.from_numpy(topo["labels"][keep_c]).to(f.device)] = 1
    keep_f = by_label[topo["component"]]
    out_v, out_f = hip_ops.mesh_submesh(v, topo["faces"], keep_f)
    info = {k: topo[k] for k in hip_ops.MESH_TOPOLOGY_COUNTS}
    info.update(components_kept=int(keep_c.sum()), components_removed=int((~keep_c).sum()), faces_removed=int(f.shape[0] - out_f.shape[0]))
    return out_v, out_f, info


SIMPLIFY_MAX_GRID = 2 ** 20


def simplify_mesh(vertices, faces, grid=None, cell=None, target_faces=None, boundary_weight=1.0, origin=None, orient=False, device=None):
    """Quadric vertex clustering on a uniform lattice with border quadrics (csrc/dudf_meshsimplify.hip): every occupied
    lattice cell becomes one vertex at the minimum of its summed plane and border quadrics, faces that keep three distinct cells survive
    (duplicates by cell set dropped, order and winding kept).  Exactly one of
      grid = n           the lattice edge is the longest extent of the finite vertices / n;
      cell = h           the lattice edge itself;
      target_faces = t   integer bisection over n in [1, 2^20] with the count-only call (at most 21 calls): the mesh of the largest n
                         tried whose face count is <= t.  The face count is NOT strictly monotone in n (a finer lattice can merge two
                         faces into one cell set that a coarser one kept apart), so this is the largest such n the bisection MEETS, not
                         the largest there is; the guarantee is faces <= t, or n == 1.
    `origin` (3 numbers) defaults to the bounding-box minimum of the finite vertices.  `boundary_weight` = 1.0 is a default, not a
    measurement (tools/bench_simplify.py prints the border's deviation for 0, 1 and 10); 0 leaves borders to erode.  Clustering can
    fold a face over or make an edge non-manifold and nothing re-winds the result: orient=True runs `orient_faces` on it.
    Returns (vertices float64, faces int64, info) on the device; info holds `hip_ops.MESH_SIMPLIFY_COUNTS` and `cell`, `grid` (None with
    cell=), `origin`, `count_calls`."""
    if sum(x is not None for x in (grid, cell, target_faces)) != 1:
        raise ValueError("simplify_mesh takes exactly one of grid, cell and target_faces")
    v, f = _device_mesh(vertices, faces, device)
    fin = v[torch.isfinite(v).all(1)]
    if fin.shape[0] == 0:
        lo, ext = [0.0, 0.0, 0.0], 0.0
    else:
        mn, mx = torch.amin(fin, 0), torch.amax(fin, 0)
        lo, ext = mn.tolist(), float((mx - mn).max())
    org = [float(x) for x in (origin.tolist() if hasattr(origin, "tolist") else origin)] if origin is not None else lo
    if len(org) != 3:
        raise ValueError("origin takes 3 numbers")
    edge = lambda n: (ext if ext > 0.0 else 1.0) / n   # noqa: E731
    calls = 0
    if cell is not None:
        h, n = float(cell), None
    elif grid is not None:
        n = int(grid)
        if not 1 <= n <= SIMPLIFY_MAX_GRID:
            raise ValueError(f"grid must lie in [1, {SIMPLIFY_MAX_GRID}]; got {grid}")
        h = edge(n)
    else:
        t = int(target_faces)
        lo_n, hi_n, n = 1, SIMPLIFY_MAX_GRID, 1                          # invariant: n is the largest lattice tried with faces <= t
        while lo_n <= hi_n:                                              # at most 21 halvings of [1, 2^20]
            mid = (lo_n + hi_n) // 2
            calls += 1
            if hip_ops.mesh_simplify_count(v, f, org, edge(mid))["faces"] <= t:
                n, lo_n = max(n, mid), mid + 1
            else:
                hi_n = mid - 1
        h = edge(n)
    out_v, out_f, info = hip_ops.mesh_simplify(v, f, org, h, boundary_weight=boundary_weight)
    if orient and out_f.shape[0]:
        out_f = orient_faces(out_v, out_f)
    info.update(cell=h, grid=n, origin=org, count_calls=calls)
    return out_v, out_f, info
