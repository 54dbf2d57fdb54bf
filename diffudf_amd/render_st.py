# coding: utf-8
"""Differential quantities the sphere tracer derives at ray hits — the query half of reference
src/render_st.py:42-65 (BASELINE config 4).  The marching loop itself (`propagate_rays`, `grad_descent`, :136-172)
runs on the device too, and so do ray set-up, orientation, colour map and shading
(`create_projectional_image`, `phong_shading`, `ward_reflectance`, :67-133, :174-245; csrc/dudf_render.hip).
`create_projectional_image_mesh` is the sphere-traced image of the ground-truth mesh (:248-281): the march against the mesh is one
kernel and the normals come from the signed distance (`MeshIndex.trace_rays`, `.signed_distance`; csrc/dudf_meshdist.hip)."""
import numpy as np
import torch
import weakref

from . import hip_ops
from .diff_operators import _source, gradient
from ._lib import DudfError


def compute_grad(inputs, outputs):
    """reference src/render_st.py:64-65"""
    return gradient(outputs, inputs)


def compute_normals_and_cd(inputs, outputs):
    """(pred_normals (1,N,3), principal directions (1,N,3,2) on the CPU) — reference src/render_st.py:57-62:
    eigh of the Hessian, normal = eigenvector of the largest eigenvalue, the other two as curvature directions."""
    model, coords = _source(outputs, inputs)
    x2 = coords.detach().reshape(-1, 3)
    _, _, _, _, V = hip_ops.query_frame(model.hip_cfg, model.flat_parameters(), x2)
    lead = coords.shape[:-1]
    normals = V[:, :, 2].reshape(lead + (3,))
    from .diff_operators import tag_field
    normals = tag_field(normals, "eig_normal", weakref.ref(model), coords)   # compute_curvature(inputs, normals) finds its way back
    return normals, V[:, :, :2].reshape(lead + (3, 2)).detach().cpu()


def compute_curvature(inputs, normals, curvature='mean', device=None):
    """reference src/render_st.py:42-55: shape operator = jacobian(normals, inputs) — third derivatives of f, obtained
    here from third-order Taylor jets along combinations of the Hessian's eigenvectors (csrc/dudf_sweep.hip
    SWEEP_FWD_J) instead of autograd through eigh.  'mean' -> trace/2, 'gaussian' -> -det [[J, n],[n^T, 0]];
    (1,N,1) CPU tensors like the reference; anything else -> None.  The sign convention of `normals` is the one
    `compute_normals_and_cd` returned (the same eigh), so the caller's re-orientation (:104-108) applies unchanged."""
    if curvature not in ('mean', 'gaussian'):
        return None
    model, coords = _source(normals, inputs)
    x2 = coords.detach().reshape(-1, 3)
    _, _, mean, gauss, _ = hip_ops.query_curvature(model.hip_cfg, model.flat_parameters(), x2,
                                                   want_shape=(curvature == 'gaussian'))
    out = mean if curvature == 'mean' else gauss
    return out.detach().cpu()[None, ..., None]


def _device_of(model, device):
    return torch.device(device) if device is not None else model.flat_parameters().device


def propagate_rays(model, rays, t0, mask_rays, network_config, rendering_config, device=None):
    """reference src/render_st.py:136-161, same signature and in-place contract: `t0` (M,3) float64 and `mask_rays` (M,)
    bool numpy arrays are updated, the bool hit mask is returned.  One upload, `max_iterations` marching iterations on
    the GPU (a host round trip every 8 of them for the `np.sum(mask_rays) > 0` test, not three copies per iteration),
    one download."""
    dev = _device_of(model, device)
    d_rays = torch.from_numpy(np.ascontiguousarray(rays, dtype=np.float64)).to(dev)
    d_t0 = torch.from_numpy(np.ascontiguousarray(t0, dtype=np.float64)).to(dev)
    d_mask = torch.from_numpy(np.ascontiguousarray(mask_rays).astype(np.uint8)).to(dev)
    with torch.cuda.device(dev):
        hits, _ = hip_ops.trace_rays(model.hip_cfg, model.flat_parameters(), d_rays, d_t0, d_mask,
                                     network_config['gt_mode'], network_config['alpha'],
                                     rendering_config['surface_threshold'], rendering_config['max_iterations'])
    t0[...] = d_t0.cpu().numpy()
    mask_rays[...] = d_mask.cpu().numpy().astype(bool)
    hits = hits.cpu().numpy().astype(bool)
    if np.sum(hits) == 0:
        raise ValueError(f"Ray tracing did not converge in {rendering_config['max_iterations']} iterations to any point at "
                         f"distance {rendering_config['surface_threshold']} or lower from surface.")
    return hits


def grad_descent(model, t0, mask_rays, network_config, rendering_config, device=None):
    """reference src/render_st.py:163-172: `gd_steps` projection steps of the hit points, in place on `t0`."""
    if rendering_config['gd_steps'] <= 0:
        return
    dev = _device_of(model, device)
    d_t0 = torch.from_numpy(np.ascontiguousarray(t0, dtype=np.float64)).to(dev)
    d_hits = torch.from_numpy(np.ascontiguousarray(mask_rays).astype(np.uint8)).to(dev)
    with torch.cuda.device(dev):
        hip_ops.descend_rays(model.hip_cfg, model.flat_parameters(), d_t0, d_hits, network_config['gt_mode'],
                             network_config['alpha'], rendering_config['gd_steps'])
    t0[...] = d_t0.cpu().numpy()


def default_colormap():
    """The (256,3) table the reference colours curvatures with (`cm.get_cmap('RdYlBu')`, src/render_st.py:89): matplotlib's
    data, fetched at call time — it is an input of this package, not a part of it."""
    try:
        import matplotlib
    except ImportError:
        raise DudfError("plotting curvatures needs a (256,3) colour table: matplotlib (RdYlBu) is not installed and no "
                        "`colormap=` was given") from None
    cmap = matplotlib.colormaps['RdYlBu']
    return np.ascontiguousarray(cmap(np.arange(cmap.N))[:, :3], dtype=np.float64)


def _lut_on(dev, colormap):
    lut = np.ascontiguousarray(colormap, dtype=np.float64)
    if lut.shape != (256, 3):
        raise DudfError(f"colormap must be a (256,3) array; got {lut.shape}")
    return torch.from_numpy(lut).to(dev)


def _wants_colormap(network_config, rendering_config):
    return network_config['gt_mode'] != 'siren' and rendering_config.get('plot_curvatures', 'none') in ('mean', 'gaussian')


def _gpu(dev, what):
    if dev.type != "cuda":
        raise DudfError(f"{what}: device must be a GPU (got {dev}); the HIP path has no CPU fallback")
    return dev


def create_projectional_image(model, rays, t0, mask_rays, network_config, rendering_config, device=None, colormap=None):
    """reference src/render_st.py:67-133, same signature (+ `colormap=`, a (256,3) table; default: matplotlib's RdYlBu): the
    (height, width, 3) float64 image of one pass.  `rays` (M,3), `t0` (M,3) float64 and `mask_rays` (M,) bool are uploaded once;
    marching, projection, the queries at the hits, orientation, colour map and shading run on the device (`hip_ops.render_traced`);
    `t0` and `mask_rays` are updated in place as `propagate_rays` / `grad_descent` do."""
    dev = _gpu(_device_of(model, device), "create_projectional_image")
    lut = None
    if _wants_colormap(network_config, rendering_config):
        lut = _lut_on(dev, default_colormap() if colormap is None else colormap)
    d_rays = torch.from_numpy(np.ascontiguousarray(rays, dtype=np.float64)).to(dev)
    d_t0 = torch.from_numpy(np.ascontiguousarray(t0, dtype=np.float64)).to(dev)
    d_mask = torch.from_numpy(np.ascontiguousarray(mask_rays).astype(np.uint8)).to(dev)
    acc = torch.zeros(d_t0.shape[0], 3, dtype=torch.float64, device=dev)
    hip_ops.render_traced(model.hip_cfg, model.flat_parameters(), d_rays, d_t0, d_mask, network_config, rendering_config, lut, acc)
    t0[...] = d_t0.cpu().numpy()
    mask_rays[...] = d_mask.cpu().numpy().astype(bool)
    return acc.cpu().numpy().reshape((rendering_config['height'], rendering_config['width'], 3))


def _shade_numpy(method, hits, samples, normals, device, color_map, **kw):
    dev = _gpu(torch.device("cuda") if device is None else torch.device(device), method)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)          # noqa: E731
    hits = np.asarray(hits).astype(bool).reshape(-1)
    d_hits = torch.from_numpy(hits.astype(np.uint8)).to(dev)
    d_samples = up(samples)
    with torch.cuda.device(dev):
        pos, _, rows, k = hip_ops.render_gather(d_hits, d_samples)
        if np.shape(normals)[0] != k:
            raise DudfError(f"{method}: {np.shape(normals)[0]} normals for {k} hits")
        acc = torch.zeros(d_samples.shape[0], 3, dtype=torch.float64, device=dev)
        extra = {n: up(v) for n, v in kw.items() if n in ("pc1", "pc2")}
        scal = {n: v for n, v in kw.items() if n not in ("pc1", "pc2")}
        hip_ops.render_shade(method, d_hits, rows, pos, up(normals), acc, color_map=None if color_map is None else up(color_map),
                             **scal, **extra)
    return acc.cpu().numpy()


def phong_shading(light_position, shininess, hits, samples, normals, color_map=None, device=None):
    """reference src/render_st.py:174-204, numpy in and out ((M,3) colours, 1.0 where `hits` is False) through
    `dudf_render_shade`.  `device=`: the GPU to run on (default: the current one)."""
    return _shade_numpy("blinn-phong", hits, samples, normals, device, color_map, light_position=light_position, shininess=shininess)


def ward_reflectance(light_position, camera_position, hits, samples, normals, alpha1, alpha2, pc1, pc2, color_map=None, device=None):
    """reference src/render_st.py:206-245 (np.nan_to_num's outcome for NaN / infinite weights included), numpy in and out."""
    return _shade_numpy("ward", hits, samples, normals, device, color_map, light_position=light_position,
                        camera_position=camera_position, alpha1=alpha1, alpha2=alpha2, pc1=pc1, pc2=pc2)


def create_projectional_image_gt(*args, **kwargs):
    """reference src/render_st.py:248-281 as written calls `phong_shading` with an argument that function no longer has, and reads
    the mesh with open3d; it keeps raising here.  `create_projectional_image_mesh` is that renderer on the device."""
    raise DudfError("create_projectional_image_gt needs open3d's RaycastingScene (ray casting against the ground-truth mesh); "
                    "it is outside this build — render the trained network with create_projectional_image, or the mesh itself "
                    "with create_projectional_image_mesh")


def load_scene(mesh, device):
    """`MeshIndex` of `mesh`: one already, (vertices, faces), the path of an OBJ (read as it is, like the reference's
    `read_triangle_mesh`), or a prefix in the sense of `diffudf_amd.mesh.prepare`: `<prefix>_t.obj`, else `<prefix>.obj` normalised."""
    import os
    from . import mesh as dmesh
    from .metrics import MeshIndex
    if isinstance(mesh, MeshIndex):
        return mesh
    if isinstance(mesh, (tuple, list)) and len(mesh) == 2:
        return MeshIndex(mesh[0], mesh[1], device=device)
    path = os.fspath(mesh)
    if os.path.isfile(path):
        v, f = dmesh.load_obj(path)
    elif os.path.isfile(path + "_t.obj"):
        v, f = dmesh.load_obj(path + "_t.obj")
    elif os.path.isfile(path + ".obj"):
        v, f = dmesh.load_obj(path + ".obj")
        v = dmesh.normalize_vertices(v)
    else:
        raise FileNotFoundError(f"no mesh at {path} ({path}_t.obj, {path}.obj)")
    return MeshIndex(v, f, device=device)


GT_GRAD_EPS = 0.0001            # reference src/render_st.py:273


def mesh_normals(scene, pos, hit_rays):
    """Normals (k,3) float64 at the hit positions pos (k,3) float64 — reference src/render_st.py:273-279: central differences of the
    SIGNED distance at float32(pos +- 1e-4 e_i), the float32 difference divided by 2e-4 as numpy forms it, normalize in float32,
    flipped where normal . ray > 0."""
    k, dev = pos.shape[0], pos.device
    grad = torch.empty(k, 3, dtype=torch.float32, device=dev)
    two_eps = torch.tensor(2 * GT_GRAD_EPS, dtype=torch.float32, device=dev)              # a tensor: a true division, not * (1 / x)
    for i in range(3):
        plus, minus = pos.clone(), pos.clone()
        plus[:, i] += GT_GRAD_EPS; minus[:, i] -= GT_GRAD_EPS                     # float64, then ONE rounding to float32 (:275-276)
        grad[:, i] = (scene.signed_distance(plus.float()) - scene.signed_distance(minus.float())) / two_eps
    normals, _, _ = hip_ops.render_orient(None, grad=grad)                        # normalize in float32
    n32 = normals.float()                                                         # exact: they are float32 values
    dot = n32[:, 0] * hit_rays[:, 0] + n32[:, 1] * hit_rays[:, 1] + n32[:, 2] * hit_rays[:, 2]
    return torch.where((dot > 0)[:, None], -normals, normals)


def mesh_pass(scene, rays, t0, mask, light_position, accumulator, specular=False, surface_eps=0.001, max_iterations=30):
    """One pass of reference src/render_st.py:255-281 on device arrays: the march against the mesh (`MeshIndex.trace_rays`; t0 and
    mask in place), `mesh_normals` at the hits, Blinn-Phong with shininess 40 (`specular`) or 0 into `accumulator` (m,3) float64
    (+=).  Returns (hits, k); 0 hits raise the reference's ValueError."""
    with torch.cuda.device(t0.device):
        hits = scene.trace_rays(rays, t0, mask, surface_eps=surface_eps, max_iterations=max_iterations)
        pos, hit_rays, rows, k = hip_ops.render_gather(hits, t0, rays)
        if k == 0:
            raise ValueError(f"Ray tracing did not converge in {max_iterations} iterations to any point at distance {surface_eps} "
                             "or lower from surface.")
        normals = mesh_normals(scene, pos, hit_rays)
        hip_ops.render_shade("blinn-phong", hits, rows, pos, normals, accumulator, light_position, shininess=40 if specular else 0)
    return hits, k


def create_projectional_image_mesh(mesh, width, height, rays, t0, mask_rays, light_position, specular=False, surface_eps=0.001,
                                   max_iterations=30, device=None):
    """The sphere-traced image of the ground-truth MESH — what reference src/render_st.py:248-281 (`create_projectional_image_gt`)
    evidently means: its march and normals operation for operation, and Blinn-Phong with shininess 40 with `specular`, 0 without.
    mesh: a path (see `load_scene`), (vertices, faces) or a `MeshIndex`.  rays (M,3), t0 (M,3) float64 and mask_rays (M,) bool numpy
    arrays; t0 and mask_rays are updated in place.  Returns the (width, height, 3) float64 image (1.0 where nothing was hit);
    raises the reference's ValueError when no ray hits."""
    dev = _gpu(torch.device("cuda:0") if device is None else torch.device(device), "create_projectional_image_mesh")
    scene = load_scene(mesh, dev)
    d_rays = torch.from_numpy(np.ascontiguousarray(rays, dtype=np.float64)).to(dev)
    d_t0 = torch.from_numpy(np.ascontiguousarray(t0, dtype=np.float64)).to(dev)
    d_mask = torch.from_numpy(np.ascontiguousarray(mask_rays).astype(np.uint8)).to(dev)
    acc = torch.zeros(d_t0.shape[0], 3, dtype=torch.float64, device=dev)
    try:
        mesh_pass(scene, d_rays, d_t0, d_mask, light_position, acc, specular, surface_eps, max_iterations)
    finally:
        t0[...] = d_t0.cpu().numpy()
        mask_rays[...] = d_mask.cpu().numpy().astype(bool)
    return acc.cpu().numpy().reshape((width, height, 3))
