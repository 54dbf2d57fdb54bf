# coding: utf-8
"""Mesh clean-up on the device — what the reference asks of trimesh behind `extract_mesh_MESHUDF` (src/render_mc.py:136-197:
`process`, duplicate and degenerate faces, `fill_holes`, Laplacian smoothing of the border), without trimesh: weld vertices on
rint(v * 10^digits), drop degenerate, duplicate and invalid faces and unused vertices, close 3- and 4-edge holes, smooth the
border.  The rules are DESIGN.md §3 "Mesh clean-up"; the kernels are csrc/dudf_meshclean.hip.  Parity with trimesh's own vertex and
face ORDER is not pinned; the result is deterministic and equals tests/meshclean_oracle.py bit for bit.

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
