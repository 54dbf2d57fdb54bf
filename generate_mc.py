#!/usr/bin/env python
# coding: utf-8
"""Mesh extraction from a trained network — reference generate_mc.py:9-67 `generate_mc`, with what this build's hot
path covers: `extract_fields` (value + gradient on the N^3 grid) feeding the extractors.

    python generate_mc.py <config.json>            keys as the reference's configs/mc_cfg.json (+ optional "luts_path")

algorithms 'meshudf' (the reference's default; SURVEY.md §8(f) row 4: the Lewiner-table marching cubes of
src/marching_cubes as host C++), 'cap' (row 2, on the device) and 'both' (what train.py asks for with gt_mode 'tanh').
MeshUDF needs the Lewiner look-up tables, which are an input, not part of this package: `luts=` / config key "luts_path"
(an .npz or the reference's `_marching_cubes_lewiner_luts.py`), $DUDF_MESHUDF_LUTS, or that module on sys.path (inside a
reference checkout: `sys.path.append('src/marching_cubes')`) — `diffudf_amd.marching_cubes.load_luts`.
The MeshUDF mesh is cleaned as the reference cleans it (weld, duplicate / degenerate faces, small holes, smoothed border): with trimesh
where it is installed, otherwise on the device (`diffudf_amd.meshclean`).
'siren' (reference generate_mc.py:56-65): `get_mesh_sdf` — the raw network values on the grid and Lewiner's marching cubes of
that signed volume, both on the device; it needs the same tables, and without them prints a message, writes nothing and returns
None (as 'both' skips its MeshUDF half), so that a training run is not lost over its mesh.
Optional key "sparse": true (with "brick", 4 or 8, and "lipschitz"; keyword `sparse=`): 'cap' on a brick-sparse narrow band
(`extract_fields_sparse` + `extract_mesh_CAP_sparse`) — for 1024^3 and up, where the dense fields do not fit.  The
other algorithms need the dense volume (MeshUDF's flood is a host walk of it) and refuse the key.
Optional keys "cap_finish": "mesh" (keyword `cap_finish=`): the CAP-UDF soup welded and wound consistently on the device
(`extract_mesh_CAP(..., finish="mesh")`); "min_component_faces" / "min_component_area_ratio": components with fewer
faces, or less than that share of the whole area, are dropped (`diffudf_amd.meshclean.remove_small_components`) — from the CAP-UDF
mesh, which is then finished as with "cap_finish", and from the device-cleaned MeshUDF mesh of 'meshudf' and 'both'.
Optional keys "simplify_target_faces" / "simplify_grid" (one of them) and "simplify_boundary_weight" (keywords of the same names): the
mesh is simplified last, on the device, by quadric vertex clustering with border quadrics (`diffudf_amd.meshclean.simplify_mesh`,
DESIGN.md §3.6c) down to at most that many faces, or on a lattice of that many cells along the longest extent, and wound again.  For
'cap' (dense or sparse) the CAP-UDF mesh is finished as with "cap_finish" first; for 'meshudf', 'both' and 'siren' the keys serve the
device-resident result (no trimesh, a GPU) and raise `DudfError` naming the key where that is not what ran.  Without these keys the
files are what they were."""
import json
import sys

import torch

from src.model import SIREN
from src.render_mc import (extract_fields, extract_fields_sparse, extract_mesh_CAP, extract_mesh_CAP_sparse, extract_mesh_MESHUDF,
                           get_mesh_sdf)
from diffudf_amd._lib import DudfError
from diffudf_amd.marching_cubes import MeshUDFError


def _component_filter(min_component_faces, min_component_area_ratio):
    """The keywords of `remove_small_components` the two optional keys stand for; empty: no filter."""
    filt = {}
    if min_component_faces is not None:
        filt["min_faces"] = int(min_component_faces)
    if min_component_area_ratio is not None:
        filt["min_area_ratio"] = float(min_component_area_ratio)
    return filt


def _without_small_components(mesh, dev, filt):
    """`mesh` (vertices, faces) without the components `filt` rejects, as the same kind of object; no filter: `mesh` itself."""
    if not filt:
        return mesh
    from diffudf_amd import meshclean
    from diffudf_amd.render_mc import _as_mesh
    v, f, _ = meshclean.remove_small_components(mesh.vertices, mesh.faces, device=dev, **filt)
    return _as_mesh(v.cpu().numpy(), f.cpu().numpy())


def _simplify_keywords(simplify_target_faces, simplify_grid, simplify_boundary_weight):
    """The keywords of `simplify_mesh` the optional keys stand for; empty: no simplification."""
    if simplify_target_faces is not None and simplify_grid is not None:
        raise ValueError("simplify_target_faces and simplify_grid exclude each other")
    if simplify_target_faces is None and simplify_grid is None:
        if simplify_boundary_weight is not None:
            raise ValueError("simplify_boundary_weight needs simplify_target_faces or simplify_grid")
        return {}
    simp = {"target_faces": int(simplify_target_faces)} if simplify_target_faces is not None else {"grid": int(simplify_grid)}
    if simplify_boundary_weight is not None:
        simp["boundary_weight"] = float(simplify_boundary_weight)
    return simp


def _simplified(mesh, dev, simp):
    """`mesh` simplified on the device (`simplify_mesh(orient=True)`); no keys: `mesh` itself.  Only a device-resident result is served:
    a trimesh object (the trimesh clean-up ran) or a CPU device raises, naming the key."""
    if not simp:
        return mesh
    from diffudf_amd import meshclean
    from diffudf_amd.render_mc import TriangleSoup
    key = "simplify_target_faces" if "target_faces" in simp else "simplify_grid"
    if dev.type != "cuda" or not isinstance(mesh, TriangleSoup):
        raise DudfError(f"'{key}' serves the device-resident mesh only ({'a CPU device' if dev.type != 'cuda' else 'the trimesh clean-up ran'})")
    v, f, _ = meshclean.simplify_mesh(mesh.vertices, mesh.faces, orient=True, device=dev, **simp)
    return TriangleSoup(v.cpu().numpy(), f.cpu().numpy())


def generate_mc(model, gt_mode, device, N, output_path, alpha=None, algorithm='meshudf', from_file=None, luts=None, sparse=False,
                brick=8, lipschitz=1.25, cap_finish=None, min_component_faces=None, min_component_area_ratio=None,
                simplify_target_faces=None, simplify_grid=None, simplify_boundary_weight=None):
    """`luts`: the Lewiner tables for MeshUDF and 'siren' (dict, path or None = look them up; see the module docstring).
    `sparse`: CAP-UDF on the narrow band of `extract_fields_sparse(..., brick=brick, lipschitz=lipschitz)`; 'cap' only.
    `cap_finish`, `min_component_faces`, `min_component_area_ratio`, `simplify_target_faces`, `simplify_grid`,
    `simplify_boundary_weight`: see the module docstring; all None: nothing changes."""
    if cap_finish not in (None, "mesh"):
        raise ValueError(f"cap_finish must be None or 'mesh'; got {cap_finish!r}")
    filt = _component_filter(min_component_faces, min_component_area_ratio)
    simp = _simplify_keywords(simplify_target_faces, simplify_grid, simplify_boundary_weight)
    finish = dict(filt, **({"simplify": simp} if simp else {})) if filt or simp else cap_finish
    if sparse and algorithm != 'cap':
        raise DudfError(f"sparse extraction serves algorithm 'cap' only; '{algorithm}' needs the dense volume")
    if from_file is not None:
        model = SIREN(n_in_features=3, n_out_features=1, hidden_layer_config=from_file["hidden_layer_nodes"],
                      w0=from_file["w0"], ww=from_file.get("ww"), activation=from_file.get('activation', 'sine'))
        model.load_state_dict(torch.load(from_file["model_path"], weights_only=True))
    dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    model.to(dev)
    if sparse:
        mesh = extract_mesh_CAP_sparse(extract_fields_sparse(model, torch.Tensor([[]]).to(dev), N, gt_mode, dev, alpha, brick=brick,
                                                             lipschitz=lipschitz), finish=finish)
        mesh.export(output_path)
        print(f'Saved to {output_path}')
        return mesh
    if algorithm in ('cap', 'both', 'meshudf'):
        u, g = extract_fields(model, torch.Tensor([[]]).to(dev), N, gt_mode, dev, alpha)
        dot = output_path.rfind('.')
        if algorithm == 'meshudf':
            _, _, mesh = extract_mesh_MESHUDF(u, g, dev, smooth_borders=True, luts=luts)
            mesh = _simplified(_without_small_components(mesh, dev, filt), dev, simp)
            mesh.export(output_path)
            print(f'Saved to {output_path}')
            return mesh
        mesh = extract_mesh_CAP(u, g, N, finish=finish)        # device tensors straight through: no host round trip
        if algorithm == 'cap':
            mesh.export(output_path)
            print(f'Saved to {output_path}')
            return mesh
        path_mu, path_cap = output_path[:dot] + '_MU' + output_path[dot:], output_path[:dot] + '_CAP' + output_path[dot:]
        mesh.export(path_cap)
        try:
            _, _, mesh_mu = extract_mesh_MESHUDF(u, g, dev, smooth_borders=True, luts=luts)
        except MeshUDFError as e:                              # no look-up tables: the CAP half is still written, and says so
            print(f'Saved to {path_cap} (MeshUDF half skipped: {e})')
            return None, mesh
        mesh_mu = _simplified(_without_small_components(mesh_mu, dev, filt), dev, simp)
        mesh_mu.export(path_mu)
        print(f'Saved to {path_mu}, {path_cap}')
        return mesh_mu, mesh
    if algorithm == 'siren':
        try:
            _, _, mesh = get_mesh_sdf(model, N=N, device=dev, luts=luts)
        except MeshUDFError as e:                              # no look-up tables: nothing is written, and the caller (a training) goes on
            print(f'{output_path} not written (signed marching cubes skipped: {e})')
            return None
        mesh = _simplified(mesh, dev, simp)
        mesh.export(output_path)
        print(f'Saved to {output_path}')
        return mesh
    raise ValueError(f"algorithm '{algorithm}' is not part of this build ('cap', 'meshudf', 'both', 'siren')")


if __name__ == "__main__":
    cfg = json.load(open(sys.argv[1]))
    generate_mc(None, cfg["gt_mode"], cfg.get("device", 0), cfg["nsamples"], cfg["output_path"], cfg.get("alpha"),
                cfg["algorithm"], from_file={"w0": cfg["w0"], "model_path": cfg["model_path"],
                                             "hidden_layer_nodes": cfg["hidden_layer_nodes"],
                                             "activation": cfg.get("activation", "sine"), "ww": cfg.get("ww")},
                luts=cfg.get("luts_path"), sparse=bool(cfg.get("sparse", False)), brick=cfg.get("brick", 8),
                lipschitz=cfg.get("lipschitz", 1.25), cap_finish=cfg.get("cap_finish"),
                min_component_faces=cfg.get("min_component_faces"), min_component_area_ratio=cfg.get("min_component_area_ratio"),
                simplify_target_faces=cfg.get("simplify_target_faces"), simplify_grid=cfg.get("simplify_grid"),
                simplify_boundary_weight=cfg.get("simplify_boundary_weight"))
