# coding: utf-8
"""Thin torch-facing layer over the C ABI: device pointers + the current HIP stream.

PyTorch is plumbing here (device memory, streams); every number is produced by the
hand-written HIP kernels in diffudf_amd/csrc.  No function in this module has a CPU path.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import NetCfg, LOSS_S1, LOSS_S2, LOSS_SIREN  # noqa: F401


BUILT_WIDTHS = (32, 64, 128, 256, 512)               # hidden widths the kernels are built for


def padded_width(hidden):
    """The built width a `hidden_layer_config` runs at: the smallest one >= its widest layer.  Zero-padding a sine MLP is
    exact: a padded unit has a zero weight row and bias (z = 0, sin = 0), the next layer's columns that read it are zero, so
    nothing it touches — value, df/dx, Hessian, any parameter gradient — changes (reference src/model.py:94-108 builds any
    list of widths; `diffudf_amd.model.SIREN` keeps the caller's shapes as strided views of the padded buffer)."""
    hidden = [int(h) for h in hidden]
    if not hidden or min(hidden) < 1:
        raise _lib.DudfError(f"hidden_layer_config must name at least one positive width; got {hidden}")
    if max(hidden) > BUILT_WIDTHS[-1]:
        raise _lib.DudfError(f"widest built layer is {BUILT_WIDTHS[-1]}; got hidden_layer_config={hidden}")
    return min(b for b in BUILT_WIDTHS if b >= max(hidden))


def make_cfg(hidden, w0=30.0, n_in=3, n_out=1, ww=None):
    """C-ABI network descriptor of SIREN(3, 1, hidden, w0, ww): L = len(hidden) layers of the padded width; `ww` = frequency of
    the SineLayers behind the first one (reference src/model.py:89-106), None / equal to w0: one frequency.  A network with a
    latent vector in front of the coordinates (n_in = 3 + k) is queried through `diffudf_amd.evaluate.evaluate`, which folds
    the latent part into the first layer's bias and arrives here with n_in = 3."""
    hidden = list(hidden)
    if n_in != 3 or n_out != 1 or len(hidden) < 1:
        raise _lib.DudfError("HIP path supports SIREN(3, 1, [...]) (3-D points, scalar field; latent-conditioned networks "
                             f"through evaluate(model, samples, latent_vec)); got n_in={n_in}, n_out={n_out}, hidden={hidden}")
    if not (float(w0) > 0) or (ww is not None and not (float(ww) > 0)):
        raise _lib.DudfError(f"SineLayer frequencies must be positive; got w0={w0}, ww={ww}")
    return NetCfg(3, len(hidden), padded_width(hidden), float(w0), 0.0 if ww is None or float(ww) == float(w0) else float(ww))


def sweeps_on_bf16(hidden, layers, w0=30.0):
    """True when this network's sweeps run on the bf16 matrix cores (bf16x6) rather than on the f32-input MFMA."""
    cfg = NetCfg(3, int(layers), int(hidden), float(w0))
    return bool(_lib.load().dudf_sweeps_bf16x6(ctypes.byref(cfg)))


def stash_mode(cfg, n=1, n_hess=0):
    """Bit mask of the stash arrays a training workspace of (cfg, n points, n_hess Hessian-path points) holds at 24 bits under the
    current options (dudf_stash_mode, include/dudf_hip.h): 0 = all fp32, 6 = R, E, C (512-wide networks; option stash = 6),
    7 = S, Q, A, Z as well (the default of 256-wide networks)."""
    return int(_lib.load().dudf_stash_mode(ctypes.byref(cfg), int(n), int(n_hess)))


OPTIONS = ("deterministic", "split", "split_quads", "sweep_family", "stash", "wgrad_family", "wgrad_tr", "pair_launch",
           "wgrad_max_workgroups", "wgrad_buffers")


def set_option(name, value):
    """dudf_set_option: a process-wide run-time option of the library (include/dudf_hip.h lists names and values).  Options that
    change the stash format or the kernel family invalidate cached workspaces (their size and layout depend on them)."""
    _call("dudf_set_option", str(name).encode(), int(value), stream=False, what=f"dudf_set_option({name!r}, {value})")
    if name != "wgrad_max_workgroups":
        _ws_cache.clear(); _qws_cache.clear()


def get_option(name):
    v = ctypes.c_int(0)
    _call("dudf_get_option", str(name).encode(), ctypes.byref(v), stream=False, what=f"dudf_get_option({name!r})")
    return int(v.value)


def reset_options():
    _call("dudf_reset_options", stream=False)
    _ws_cache.clear(); _qws_cache.clear()


class options:
    """`with hip_ops.options(stash=0, split=0): ...` — set options for a block and restore what was there before."""

    def __init__(self, **kw):
        self.kw, self.old = kw, {}

    def __enter__(self):
        for k, v in self.kw.items():
            self.old[k] = get_option(k)
            set_option(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            set_option(k, v)
        return False


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _call(name, *args, dev=None, stream=True, what=None):
    """One C-ABI call: `name(*args[, current stream])` under the device guard of `dev` (None: no guard); a non-zero return raises,
    named after the symbol (or `what`)."""
    fn = getattr(_lib.load(), name)
    if stream:
        args += (_stream(),)
    if dev is None:
        rc = fn(*args)
    else:
        with torch.cuda.device(dev):
            rc = fn(*args)
    _lib.check(rc, what or name)


def _bytes(name, *args, err=-1):
    """A byte (or element) count of the library; it answers 0 (or less) for arguments it refuses."""
    n = int(getattr(_lib.load(), name)(*args))
    if n <= 0:
        _lib.check(err, name)
    return n


def _scratch(nbytes, device):
    """256-byte-aligned device scratch of the C ABI's (workspace, bytes) pairs."""
    buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
    assert buf.data_ptr() % 256 == 0
    return buf


def _workspace(device, name, *args, err=-1):
    """(scratch, its byte count) for the stage whose size `name(*args)` publishes."""
    nbytes = _bytes(name, *args, err=err)
    return _scratch(nbytes, device), nbytes


def _tensor(t, what, dtype, shape=None, convert=False):
    """`t` as the C ABI reads it: a contiguous CUDA tensor of `dtype` whose dimensions behind the first are `shape` (None: any
    shape).  convert: another dtype or stride is converted, otherwise it is refused."""
    if not torch.is_tensor(t) or t.device.type != "cuda":
        raise _lib.DudfError(f"{what} must be a CUDA tensor (got {getattr(t, 'device', type(t).__name__)}); the HIP path has no CPU fallback")
    if shape is not None and (t.dim() != 1 + len(shape) or tuple(t.shape[1:]) != tuple(shape)):
        raise _lib.DudfError(f"{what} must have shape (n,{','.join(str(d) for d in shape or ())}); got {tuple(t.shape)}")
    if convert:
        return t.to(dtype).contiguous()
    if t.dtype != dtype or not t.is_contiguous():
        raise _lib.DudfError(f"{what} must be a contiguous {str(dtype).replace('torch.', '')} tensor; got {t.dtype} {tuple(t.shape)}")
    return t


def theta_count(cfg):
    return _bytes("dudf_theta_count", ctypes.byref(cfg))


_theta_counts = {}


def _theta(cfg, theta, convert=True):
    """theta as the C ABI takes it: flat fp32 on the GPU with exactly this network's (padded) parameter count — the library
    indexes it by the layout of `cfg` and cannot know the length of the buffer behind a pointer.  convert=False (the training
    path): checked only."""
    if convert:
        theta = _tensor(theta, "theta", torch.float32, convert=True)
    key = (cfg.n_hidden_layers, cfg.hidden)
    n = _theta_counts.get(key)
    if n is None:
        n = _theta_counts[key] = theta_count(cfg)
    if theta.numel() != n or theta.dtype != torch.float32 or theta.device.type != "cuda":
        raise _lib.DudfError(f"theta must be {n} fp32 elements on the GPU for SIREN(3, 1, [{cfg.hidden}]*{cfg.n_hidden_layers}); got "
                             f"{theta.numel()} x {theta.dtype} on {theta.device}")
    return theta


class Workspace:
    """Caller-owned scratch for one (cfg, n_points, n_hess).  Holds the stash between forward and backward."""
    _bytes_symbol = "dudf_workspace_bytes_hess"

    def __init__(self, cfg, n, device, n_hess=0):
        self.cfg, self.n, self.n_hess = cfg, int(n), int(n_hess)
        self.buf, self.nbytes = _workspace(device, self._bytes_symbol, ctypes.byref(cfg), self.n, self.n_hess)


class QueryWorkspace(Workspace):
    """The smaller scratch the value / df/dx / Hessian queries need (no adjoint stash)."""
    _bytes_symbol = "dudf_workspace_bytes_query"


_ws_cache = {}
_qws_cache = {}


def query_workspace_for(cfg, n, device, n_hess=0):
    key = (cfg.n_hidden_layers, cfg.hidden, cfg.w0, int(n), str(device), int(n_hess))
    ws = _qws_cache.get(key)
    if ws is None:
        _qws_cache.clear()
        ws = _qws_cache[key] = QueryWorkspace(cfg, n, device, n_hess)
    return ws


def workspace_for(cfg, n, device, n_hess=0):
    key = (cfg.n_hidden_layers, cfg.hidden, cfg.w0, int(n), str(device), int(n_hess))
    ws = _ws_cache.get(key)
    if ws is None:
        for k in [k for k in _ws_cache if k[:3] == key[:3] and k[4] == key[4]]:
            del _ws_cache[k]                      # one live workspace per network: they are large
        ws = _ws_cache[key] = Workspace(cfg, n, device, n_hess)
    return ws


def query(cfg, theta, x, want_grad=True, ws=None):
    """f (n,), df/dx (n,3) or None.  Reference: src/evaluate.py:26-32 per chunk."""
    x = _tensor(x, "x", torch.float32, convert=True).view(-1, 3)
    theta = _theta(cfg, theta)
    n = x.shape[0]
    ws = ws or query_workspace_for(cfg, n, x.device)
    f = torch.empty(n, dtype=torch.float32, device=x.device)
    g = torch.empty(n, 3, dtype=torch.float32, device=x.device) if want_grad else None
    _call("dudf_query", ctypes.byref(cfg), _ptr(theta), _ptr(x), n, _ptr(f), _ptr(g), _ptr(ws.buf), ws.nbytes)
    return f, g


def query_hessian(cfg, theta, x, ws=None):
    """f (n,), df/dx (n,3), Hessian (n,3,3) [i][k] = d(df/dx_i)/dx_k.  Reference: src/evaluate.py:26-35."""
    x = _tensor(x, "x", torch.float32, convert=True).view(-1, 3)
    theta = _theta(cfg, theta)
    n = x.shape[0]
    ws = ws or query_workspace_for(cfg, n, x.device, n_hess=n)
    f = torch.empty(n, dtype=torch.float32, device=x.device)
    g = torch.empty(n, 3, dtype=torch.float32, device=x.device)
    h = torch.empty(n, 3, 3, dtype=torch.float32, device=x.device)
    _call("dudf_query_hessian", ctypes.byref(cfg), _ptr(theta), _ptr(x), n, _ptr(f), _ptr(g), _ptr(h), _ptr(ws.buf), ws.nbytes)
    return f, g, h


def query_frame(cfg, theta, x, ws=None):
    """f, df/dx, Hessian, eigenvalues (n,3) ascending, eigenvectors (n,3,3) as columns — eigh of the Hessian's
    lower triangle (reference src/render_st.py:57-62)."""
    x = _tensor(x, "x", torch.float32, convert=True).view(-1, 3)
    theta = _theta(cfg, theta)
    n = x.shape[0]
    ws = ws or query_workspace_for(cfg, n, x.device, n_hess=n)
    dev = x.device
    f = torch.empty(n, dtype=torch.float32, device=dev); g = torch.empty(n, 3, dtype=torch.float32, device=dev)
    h = torch.empty(n, 3, 3, dtype=torch.float32, device=dev); lam = torch.empty(n, 3, dtype=torch.float32, device=dev)
    v = torch.empty(n, 3, 3, dtype=torch.float32, device=dev)
    _call("dudf_query_frame", ctypes.byref(cfg), _ptr(theta), _ptr(x), n, _ptr(f), _ptr(g), _ptr(h), _ptr(lam), _ptr(v),
          _ptr(ws.buf), ws.nbytes)
    return f, g, h, lam, v


def query_curvature(cfg, theta, x, want_shape=False, chunk=65536):
    """Eigen-frame of the Hessian and the curvature of its top-eigenvector field (reference src/render_st.py:42-62):
    lam (n,3), V (n,3,3) [normal = V[:,:,2]], mean (n,), and with want_shape also gaussian (n,) and the shape operator
    J (n,3,3) = d normal_i / d x_k; (None, None) otherwise.  Runs in chunks so the scratch stays a few GB."""
    x = _tensor(x, "x", torch.float32, convert=True).view(-1, 3)
    theta = _theta(cfg, theta)
    n, dev = x.shape[0], x.device
    lam = torch.empty(n, 3, dtype=torch.float32, device=dev); v = torch.empty(n, 3, 3, dtype=torch.float32, device=dev)
    mean = torch.empty(n, dtype=torch.float32, device=dev)
    gauss = torch.empty(n, dtype=torch.float32, device=dev) if want_shape else None
    shape = torch.empty(n, 3, 3, dtype=torch.float32, device=dev) if want_shape else None
    m = min(max(n, 1), int(chunk))
    buf, nbytes = _workspace(dev, "dudf_workspace_bytes_curvature", ctypes.byref(cfg), m)
    for s in range(0, n, m):
        e = min(s + m, n)
        _call("dudf_query_curvature", ctypes.byref(cfg), _ptr(theta), _ptr(x[s:e]), e - s, _ptr(lam[s:e]), _ptr(v[s:e]),
              _ptr(mean[s:e]), _ptr(gauss[s:e]) if want_shape else None, _ptr(shape[s:e]) if want_shape else None, _ptr(buf),
              nbytes)
    return lam, v, mean, gauss, shape


INVERSE_MODES = {"tanh": 0, "siren": 1, "squared": 2}


def trace_rays(cfg, theta, rays, t0, mask, gt_mode, alpha, surface_threshold, max_iterations, check_every=8, min_step=0.01):
    """The marching loop of reference src/render_st.py:136-161 on the device.  rays (m,3), t0 (m,3) float64 CUDA tensors,
    mask (m,) uint8; t0 and mask are updated in place.  Returns (hits (m,) uint8, iterations executed)."""
    theta = _theta(cfg, theta)
    m = t0.shape[0]
    for name, t, dt in (("rays", rays, torch.float64), ("t0", t0, torch.float64), ("mask", mask, torch.uint8)):
        _tensor(t, f"trace_rays: {name}", dt)
    hits = torch.empty(m, dtype=torch.uint8, device=t0.device)
    ws = query_workspace_for(cfg, m, t0.device)
    done = ctypes.c_int(0)
    _call("dudf_trace_rays", ctypes.byref(cfg), _ptr(theta), _ptr(rays), _ptr(t0), _ptr(mask), _ptr(hits), m,
          INVERSE_MODES[gt_mode], float(alpha), float(min_step), float(surface_threshold), int(max_iterations), int(check_every),
          ctypes.byref(done), _ptr(ws.buf), ws.nbytes)
    return hits, done.value


def descend_rays(cfg, theta, t0, hits, gt_mode, alpha, gd_steps, min_step=0.01):
    """`grad_descent` of reference src/render_st.py:163-172 on the device; t0 (m,3) float64 updated in place."""
    theta = _theta(cfg, theta)
    m = t0.shape[0]
    ws = query_workspace_for(cfg, m, t0.device)
    _call("dudf_descend_rays", ctypes.byref(cfg), _ptr(theta), _ptr(t0), _ptr(hits), m, INVERSE_MODES[gt_mode], float(alpha),
          float(min_step), int(gd_steps), _ptr(ws.buf), ws.nbytes)


def project_points(cfg, theta, points, gt_mode, alpha, num_steps=5, surf_thresh=0.01):
    """The inner loop of reference src/render_pc.py:43-56 on the device: `points` (n,3) float64 CUDA tensor, moved in place by
    `num_steps` projection steps.  Returns (last_step (n,) float64, unit_grad (n,3) float64 = normalize(grad) before the last move,
    pre_pos (n,3) float32 = the position the network saw at the last step, accept (n,) uint8 = in the closed domain after the
    move and last step < surf_thresh)."""
    theta = _theta(cfg, theta)
    points = _tensor(points, "project_points: points", torch.float64, (3,))
    n, dev = points.shape[0], points.device
    last = torch.empty(n, dtype=torch.float64, device=dev); unit = torch.empty(n, 3, dtype=torch.float64, device=dev)
    pre = torch.empty(n, 3, dtype=torch.float32, device=dev); acc = torch.empty(n, dtype=torch.uint8, device=dev)
    ws = query_workspace_for(cfg, n, dev)
    _call("dudf_project_points", ctypes.byref(cfg), _ptr(theta), _ptr(points), n, int(num_steps), INVERSE_MODES[gt_mode],
          float(alpha), float(surf_thresh), _ptr(last), _ptr(unit), _ptr(pre), _ptr(acc), _ptr(ws.buf), ws.nbytes, dev=dev)
    return last, unit, pre, acc


def pointcloud_append(flags, src_a, dst_a, counter, src_b=None, dst_b=None, src_f=None, out_f=None, quota=None):
    """`dst = np.vstack((dst, src[flags]))` on the device (reference src/render_pc.py:58-65): the flagged rows of src_a (and
    src_b) (n,3) float64 go, in their order, behind row counter[0] of dst_a (dst_b); the flagged rows of src_f (n,3) float32 to
    out_f from row 0.  counter: int64 CUDA tensor of 4 — [0] rows held (advanced), [1] rows added by this call, [2] rows held
    before it.  Nothing is added once counter[0] >= quota (default: never) or when the rows would not fit into dst_a."""
    flags = _tensor(flags, "pointcloud_append: flags", torch.uint8)
    n, dev = flags.shape[0], flags.device
    src_a = _tensor(src_a, "pointcloud_append: src_a", torch.float64, (3,))
    dst_a = _tensor(dst_a, "pointcloud_append: dst_a", torch.float64, (3,))
    if (src_b is None) != (dst_b is None) or (src_f is None) != (out_f is None):
        raise _lib.DudfError("pointcloud_append: src_b / dst_b and src_f / out_f come in pairs")
    if src_b is not None:
        src_b = _tensor(src_b, "pointcloud_append: src_b", torch.float64, (3,))
        dst_b = _tensor(dst_b, "pointcloud_append: dst_b", torch.float64, (3,))
    if src_f is not None:
        _tensor(src_f, "pointcloud_append: src_f", torch.float32); _tensor(out_f, "pointcloud_append: out_f", torch.float32)
        if out_f.shape[0] < n:
            raise _lib.DudfError("pointcloud_append: out_f must have a row for every source row")
    if _tensor(counter, "pointcloud_append: counter", torch.int64).numel() != 4:
        raise _lib.DudfError("pointcloud_append: counter must be an int64 CUDA tensor of 4")
    if src_a.shape[0] != n or (src_b is not None and (src_b.shape[0] != n or dst_b.shape[0] != dst_a.shape[0])) or \
            (src_f is not None and src_f.shape[0] != n):
        raise _lib.DudfError("pointcloud_append: row counts of flags and sources differ")
    ws, nbytes = _workspace(dev, "dudf_pointcloud_append_workspace_bytes", n)
    _call("dudf_pointcloud_append", _ptr(flags), n, _ptr(src_a), _ptr(src_b), _ptr(src_f), _ptr(dst_a), _ptr(dst_b), _ptr(out_f),
          dst_a.shape[0], (1 << 62) if quota is None else int(quota), _ptr(counter), _ptr(ws), nbytes, dev=dev)


class PointCloudState:
    """Caller-owned state of `pointcloud_round`: surface points and normals (2 * num_points rows, float64), the device row
    counter and the round workspace."""

    def __init__(self, cfg, num_points, device):
        self.cfg, self.num_points = cfg, int(num_points)
        self.capacity = max(2 * self.num_points, 1)
        self.points = torch.zeros(self.capacity, 3, dtype=torch.float64, device=device)
        self.normals = torch.zeros(self.capacity, 3, dtype=torch.float64, device=device)
        self.counter = torch.zeros(4, dtype=torch.int64, device=device)
        self.buf, self.nbytes = _workspace(device, "dudf_pointcloud_workspace_bytes", ctypes.byref(cfg), self.num_points)
        self.rounds = 0

    def count(self):
        return int(self.counter[0].item())

    def proposals(self):
        """(num_points,3) float64: the rows the last round proposed, before any move (diagnostic; reference :36-39)."""
        out = torch.empty(self.num_points, 3, dtype=torch.float64, device=self.points.device)
        _call("dudf_pointcloud_read_proposals", ctypes.byref(self.cfg), self.num_points, _ptr(out), _ptr(self.buf), self.nbytes,
              dev=self.points.device)
        return out


def pointcloud_round(cfg, theta, state, gt_mode, alpha, num_steps=5, surf_thresh=0.01, rand=None, seed=0, want_count=True):
    """One round of reference src/render_pc.py:33-68 on `state` (propose -> project -> ordered append -> normals).  rand: float64
    CUDA tensor with the host-drawn numbers of this round (layout: include/dudf_hip.h) or None for the in-kernel generator keyed by
    (seed, round).  Returns the host copy of the counter [rows held, rows added, rows held before] or None (want_count=False)."""
    theta = _theta(cfg, theta)
    if rand is not None:
        _tensor(rand, "pointcloud_round: rand", torch.float64)
        half = state.num_points // 2
        if rand.numel() not in (3 * state.num_points, 7 * half):
            raise _lib.DudfError(f"pointcloud_round: rand has {rand.numel()} numbers; a round of {state.num_points} points takes "
                                 f"{3 * state.num_points} (first form) or {7 * half}")
    hc = (ctypes.c_int64 * 4)() if want_count else None
    _call("dudf_pointcloud_round", ctypes.byref(cfg), _ptr(theta), state.num_points, int(num_steps), INVERSE_MODES[gt_mode],
          float(alpha), float(surf_thresh), _ptr(rand), 0 if rand is None else rand.numel(), int(seed) & ((1 << 64) - 1),
          state.rounds, _ptr(state.points), _ptr(state.normals), state.capacity, _ptr(state.counter), hc, _ptr(state.buf),
          state.nbytes, dev=state.points.device)
    state.rounds += 1
    return list(hc)[:3] if want_count else None


def grid_fields(cfg, theta, grid_n, start, count, gt_mode, alpha, out_df, out_vec, ws=None):
    """Fills out_df[start:start+count], out_vec[start:start+count] (device tensors over the flattened N^3 grid);
    returns the device int32 counter of points that need the Hessian-eigenvector fallback."""
    theta = _theta(cfg, theta)
    ws = ws or query_workspace_for(cfg, count, theta.device)
    flag = torch.zeros(1, dtype=torch.int32, device=theta.device)
    df = out_df[start:start + count]
    vec = out_vec[start:start + count]
    _call("dudf_grid_fields", ctypes.byref(cfg), _ptr(theta), int(grid_n), int(start), int(count), INVERSE_MODES[gt_mode],
          float(alpha), _ptr(df), _ptr(vec), _ptr(flag), _ptr(ws.buf), ws.nbytes)
    return flag


def grid_values(cfg, theta, grid_n, start, count, out_f, ws=None):
    """Fills out_f[start:start+count] (a device tensor over the flattened N^3 grid) with the raw network output, sign kept
    (`dudf_grid_values`: the forward sweep only)."""
    theta = _theta(cfg, theta)
    ws = ws or query_workspace_for(cfg, count, theta.device)
    _call("dudf_grid_values", ctypes.byref(cfg), _ptr(theta), int(grid_n), int(start), int(count), _ptr(out_f[start:start + count]),
          _ptr(ws.buf), ws.nbytes, dev=theta.device)


def mc_lewiner_extract(volume, level, lut_data, lut_offsets, lut_dims):
    """Lewiner marching cubes of a signed device volume (nz, ny, nx) at `level` (`dudf_mc_lewiner_count` / `_emit`):
    (vertices (V,3) float32 in x-y-z grid units, faces (T,3) int32, raw normal sums (V,3) float32, values (V,) float32) device
    tensors, bit for bit what `marching_cubes.marching_cubes_sdf` gives for the same numbers on the host.  lut_data: the packed
    tables as an int8 device tensor, lut_offsets / lut_dims: their numpy descriptors (`marching_cubes._pack_luts`).  One host
    sync for the two output sizes; nothing is launched for an empty result."""
    volume = _tensor(volume, "volume", torch.float32, convert=True)
    lut_data = _tensor(lut_data, "lut_data", torch.int8)
    if volume.dim() != 3 or lut_data.device != volume.device:
        raise _lib.DudfError(f"mc_lewiner_extract: a (nz, ny, nx) volume and tables on its device expected, got {tuple(volume.shape)}")
    nz, ny, nx = volume.shape
    dev = volume.device
    ws, nbytes = _workspace(dev, "dudf_mc_lewiner_workspace_bytes", nz, ny, nx)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    head = (_ptr(volume), nz, ny, nx, float(level), _ptr(lut_data), ctypes.c_void_p(lut_offsets.ctypes.data),
            ctypes.c_void_p(lut_dims.ctypes.data), len(lut_offsets))
    _call("dudf_mc_lewiner_count", *head, _ptr(counts), _ptr(ws), nbytes, dev=dev)
    nv, nt = [int(v) for v in counts.tolist()]
    if nv >= 1 << 31:
        raise _lib.DudfError(f"mc_lewiner_extract: {nv} vertices do not fit int32 faces")
    verts = torch.empty(nv, 3, dtype=torch.float32, device=dev); faces = torch.empty(nt, 3, dtype=torch.int32, device=dev)
    normals = torch.empty(nv, 3, dtype=torch.float32, device=dev); values = torch.empty(nv, dtype=torch.float32, device=dev)
    if nv and nt:
        _call("dudf_mc_lewiner_emit", *head, _ptr(verts), _ptr(faces), _ptr(normals), _ptr(values), _ptr(ws), nbytes, dev=dev)
    return verts, faces, normals, values


def capudf_extract(ndf, grad, threshold=0.008, want_cells=False):
    """CAP-UDF cell extraction (reference src/render_mc.py:201-256) on device fields ndf (N,N,N), grad (N,N,N,3):
    (vertices (V,3) float64 in [-1,1]^3, triangles (T,3) int64[, cells (C,3) int64]) device tensors.  One host sync
    for the three output sizes."""
    ndf = _tensor(ndf, "ndf", torch.float32, convert=True); grad = _tensor(grad, "grad", torch.float32, convert=True)
    n = ndf.shape[0]
    if ndf.shape != (n, n, n) or grad.shape != (n, n, n, 3):
        raise _lib.DudfError(f"capudf_extract: ndf (N,N,N) and grad (N,N,N,3) expected, got {tuple(ndf.shape)}, {tuple(grad.shape)}")
    dev = ndf.device
    ws, nbytes = _workspace(dev, "dudf_capudf_workspace_bytes", n)
    counts = torch.zeros(3, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _call("dudf_capudf_count", _ptr(ndf), _ptr(grad), n, float(threshold), _ptr(counts), _ptr(ws), nbytes)
        nc, nv, nt = [int(v) for v in counts.tolist()]
        verts = torch.empty(nv, 3, dtype=torch.float64, device=dev)
        tris = torch.empty(nt, 3, dtype=torch.int64, device=dev)
        cells = torch.empty(nc, 3, dtype=torch.int64, device=dev) if want_cells else None
        if nc:
            _call("dudf_capudf_emit", _ptr(ndf), _ptr(grad), n, float(threshold), _ptr(verts), _ptr(tris), _ptr(cells), _ptr(ws),
                  nbytes)
    return (verts, tris, cells) if want_cells else (verts, tris)


# ---- the brick-sparse narrow band (dudf_sparsegrid.hip; layout and rules: include/dudf_hip.h) ----------------------
def sparse_dims(grid_n, brick):
    """(m, nb, nl): cells per side, cell bricks per side, storage-lattice bricks per side; the coarse lattice has nb + 1 points."""
    grid_n, brick = int(grid_n), int(brick)
    if brick not in (4, 8) or grid_n < 2:
        _lib.check(-1, f"sparse grid (N = {grid_n}, brick = {brick}: N >= 2 and a brick edge of 4 or 8)")
    m = grid_n - 1
    return m, -(-m // brick), m // brick + 1


def sparse_bound(grid_n, brick, threshold, lipschitz):
    """The selection bound of a brick for an L-Lipschitz df, in double: threshold + L * half a brick diagonal."""
    return float(threshold) + float(lipschitz) * (math.sqrt(3.0) / 2.0) * int(brick) * (2.0 / (int(grid_n) - 1))


def grid_fields_lattice(cfg, theta, grid_n, brick, start, count, gt_mode, alpha, out_df, out_vec=None, ws=None):
    """Fills out_df[start:start+count] (and out_vec, when given) over the flattened (nb + 1)^3 coarse lattice at fine indices
    min(c * brick, N - 1); out_vec None: the forward sweep only.  Returns the fallback counter as `grid_fields` (None without out_vec)."""
    theta = _theta(cfg, theta)
    ws = ws or query_workspace_for(cfg, count, theta.device)
    flag = torch.zeros(1, dtype=torch.int32, device=theta.device) if out_vec is not None else None
    _call("dudf_grid_fields_lattice", ctypes.byref(cfg), _ptr(theta), int(grid_n), int(brick), int(start), int(count),
          INVERSE_MODES[gt_mode], float(alpha), _ptr(out_df[start:start + count]),
          _ptr(out_vec[start:start + count] if out_vec is not None else None), _ptr(flag), _ptr(ws.buf), ws.nbytes, dev=theta.device)
    return flag


def sparse_select(coarse_df, grid_n, brick, bound):
    """Brick selection (`dudf_sparse_select`) from df on the coarse lattice: (slot (nl,nl,nl) int32, stored_ids, candidate_ids) device
    tensors, the id lists ascending int32 and cut to their counts — the one host read-back of the sparse extraction."""
    m, nb, nl = sparse_dims(grid_n, brick)
    coarse_df = _tensor(coarse_df, "coarse_df", torch.float32, convert=True)
    if coarse_df.numel() != (nb + 1) ** 3:
        raise _lib.DudfError(f"sparse_select: {(nb + 1) ** 3} lattice values expected for N = {grid_n}, brick = {brick}; got {coarse_df.numel()}")
    dev = coarse_df.device
    ws, nbytes = _workspace(dev, "dudf_sparse_select_bytes", int(grid_n), int(brick), err=-4)
    slot = torch.empty(nl, nl, nl, dtype=torch.int32, device=dev)
    stored = torch.empty(nl ** 3, dtype=torch.int32, device=dev); cands = torch.empty(nl ** 3, dtype=torch.int32, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    _call("dudf_sparse_select", _ptr(coarse_df), int(grid_n), int(brick), float(bound), _ptr(slot), _ptr(stored), _ptr(cands),
          _ptr(counts), _ptr(ws), nbytes, dev=dev)
    ns, nc = [int(v) for v in counts.tolist()]
    return slot, stored[:ns].clone(), cands[:nc].clone()


def grid_fields_bricks(cfg, theta, grid_n, brick, stored_ids, first, count, gt_mode, alpha, out_df, out_vec, ws=None):
    """Fills the slots first .. first+count-1 of out_df (slots, B, B, B) and out_vec (slots, B, B, B, 3) with the fields of the bricks
    stored_ids[first:first+count]; returns the device int32 counter of points that need the Hessian-eigenvector fallback."""
    theta = _theta(cfg, theta)
    npts = int(count) * int(brick) ** 3
    ws = ws or query_workspace_for(cfg, npts, theta.device)
    flag = torch.zeros(1, dtype=torch.int32, device=theta.device)
    _call("dudf_grid_fields_bricks", ctypes.byref(cfg), _ptr(theta), int(grid_n), int(brick), _ptr(stored_ids[first:first + count]),
          int(count), INVERSE_MODES[gt_mode], float(alpha), _ptr(out_df[first:first + count]), _ptr(out_vec[first:first + count]),
          _ptr(flag), _ptr(ws.buf), ws.nbytes, dev=theta.device)
    return flag


def capudf_sparse_extract(df, vec, slot, candidate_ids, grid_n, brick, threshold=0.008, want_cells=False, want_counts=False):
    """`capudf_extract` on brick storage: df (slots,B,B,B), vec (slots,B,B,B,3), the slot table and the ascending candidate list of
    `sparse_select`.  Same outputs (cells: GLOBAL cell indices, candidate bricks ascending, local (i, j, k) order inside each); one
    host sync for the three output sizes.  want_counts: the (cells, vertices, triangles) of the count call come back last."""
    m, nb, nl = sparse_dims(grid_n, brick)
    df = _tensor(df, "df", torch.float32, (brick,) * 3); vec = _tensor(vec, "vec", torch.float32, (brick,) * 3 + (3,))
    slot = _tensor(slot, "slot", torch.int32); candidate_ids = _tensor(candidate_ids, "candidate_ids", torch.int32)
    if slot.numel() != nl ** 3 or vec.shape[0] != df.shape[0] or candidate_ids.dim() != 1:
        raise _lib.DudfError(f"capudf_sparse_extract: a slot table of {nl}^3 entries and df / vec of the same slots expected, got "
                             f"{tuple(slot.shape)}, {tuple(df.shape)}, {tuple(vec.shape)}")
    dev = df.device
    ncand = int(candidate_ids.numel())
    counts = torch.zeros(3, dtype=torch.int64, device=dev)
    nc = nv = nt = 0
    if ncand:
        ws, nbytes = _workspace(dev, "dudf_capudf_sparse_workspace_bytes", int(grid_n), int(brick), ncand, err=-4)
        head = (_ptr(df), _ptr(vec), _ptr(slot), _ptr(candidate_ids), ncand, int(grid_n), int(brick), float(threshold))
        _call("dudf_capudf_sparse_count", *head, _ptr(counts), _ptr(ws), nbytes, dev=dev)
        nc, nv, nt = [int(v) for v in counts.tolist()]
    verts = torch.empty(nv, 3, dtype=torch.float64, device=dev)
    tris = torch.empty(nt, 3, dtype=torch.int64, device=dev)
    cells = torch.empty(nc, 3, dtype=torch.int64, device=dev) if want_cells else None
    if nc:
        _call("dudf_capudf_sparse_emit", *head, _ptr(verts), _ptr(tris), _ptr(cells), _ptr(ws), nbytes, dev=dev)
    out = (verts, tris) + ((cells,) if want_cells else ())
    return out + ((nc, nv, nt),) if want_counts else out


MESH_CLEAN_COUNTS = ("vertices", "faces", "welded", "unreferenced", "duplicate_faces", "degenerate_faces", "holes3", "holes4",
                     "invalid_faces")


def _mesh(vertices, faces):
    vertices = _tensor(vertices, "vertices", torch.float64, (3,), convert=True)
    faces = _tensor(faces, "faces", torch.int64, (3,), convert=True)
    if faces.device != vertices.device:
        raise _lib.DudfError("vertices and faces must be on one device")
    return vertices, faces


def mesh_clean_round(vertices, faces, digits=8, fill_holes=False):
    """One clean-up round of a device mesh (`dudf_mesh_clean_count` / `_emit`; the rules: DESIGN.md §3 "Mesh clean-up"): invalid faces
    dropped, vertices welded on rint(v * 10^digits), faces remapped and pruned (degenerate, duplicate), unused vertices dropped, and
    with fill_holes the 3- and 4-edge holes of that result closed.  (vertices (V',3) float64, faces (F',3) int64, counts: a dict over
    MESH_CLEAN_COUNTS).  One host sync for the counts; nothing is emitted for an empty result, and a round that changes nothing
    returns its inputs."""
    vertices, faces = _mesh(vertices, faces)
    dev = vertices.device
    V, F = vertices.shape[0], faces.shape[0]
    ws, nbytes = _workspace(dev, "dudf_mesh_clean_workspace_bytes", V, F, err=-4)
    counts = torch.zeros(len(MESH_CLEAN_COUNTS), dtype=torch.int64, device=dev)
    head = (_ptr(vertices), V, _ptr(faces), F, int(digits), int(bool(fill_holes)))
    _call("dudf_mesh_clean_count", *head, _ptr(counts), _ptr(ws), nbytes, dev=dev)
    c = dict(zip(MESH_CLEAN_COUNTS, (int(v) for v in counts.tolist())))
    nv, nf = c["vertices"], c["faces"]
    if (nv, nf) == (V, F) and not c["holes3"] and not c["holes4"]:        # nothing dropped, nothing added: the identity
        return vertices, faces, c
    out_v = torch.empty(nv, 3, dtype=torch.float64, device=dev); out_f = torch.empty(nf, 3, dtype=torch.int64, device=dev)
    if nv and nf:
        _call("dudf_mesh_clean_emit", *head, _ptr(out_v), _ptr(out_f), _ptr(ws), nbytes, dev=dev)
    return out_v, out_f, c


def mesh_border_edges(faces, n_vertices):
    """(E,2) int64 device tensor: the undirected edges (u < w) that exactly one face uses, ascending (`dudf_mesh_border_count` /
    `_edges`).  One host sync for E."""
    faces = _tensor(faces, "faces", torch.int64, (3,), convert=True)
    dev = faces.device
    V, F = int(n_vertices), faces.shape[0]
    ws, nbytes = _workspace(dev, "dudf_mesh_border_workspace_bytes", V, F, err=-4)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    _call("dudf_mesh_border_count", V, _ptr(faces), F, _ptr(count), _ptr(ws), nbytes, dev=dev)
    edges = torch.empty(int(count.item()), 2, dtype=torch.int64, device=dev)
    if edges.shape[0]:
        _call("dudf_mesh_border_edges", V, _ptr(faces), F, _ptr(edges), _ptr(ws), nbytes, dev=dev)
    return edges


def mesh_smooth_borders(vertices, faces, iterations=5, lam=0.3):
    """A new (V,3) float64 device tensor: `iterations` Jacobi steps v += lam * (mean(border neighbours) - v) on the border vertices
    of the mesh (`dudf_mesh_smooth_borders`; reference src/render_mc.py:169-197).  No host sync."""
    vertices, faces = _mesh(vertices, faces)
    out = vertices.clone()
    V, F = out.shape[0], faces.shape[0]
    ws, nbytes = _workspace(out.device, "dudf_mesh_border_workspace_bytes", V, F, err=-4)
    _call("dudf_mesh_smooth_borders", _ptr(out), V, _ptr(faces), F, int(iterations), float(lam), _ptr(ws), nbytes, dev=out.device)
    return out


MESH_TOPOLOGY_COUNTS = ("components", "forest_edges", "manifold_edges", "border_edges", "nonmanifold_edges", "ignored_faces",
                        "flipped_faces", "inconsistent_edges")


def mesh_topology(faces, n_vertices, vertices=None):
    """Winding and components of a device mesh (`dudf_mesh_topology`; the rules: DESIGN.md §3.6b).  faces (F,3) int64, vertices None
    or (V,3) float64 (then the integer areas are filled).  Returns (oriented faces (F,3) int64, component (F,) int64, flip (F,) uint8,
    component_faces (F,) int64, component_area_q (F,) int64 holding the bits of the uint64 sums, counts: a dict
    over MESH_TOPOLOGY_COUNTS).  The Borůvka rounds read one word back each; the counts are one more host sync."""
    faces = _tensor(faces, "faces", torch.int64, (3,), convert=True)
    dev = faces.device
    V, F = int(n_vertices), faces.shape[0]
    if vertices is not None:
        vertices = _tensor(vertices, "vertices", torch.float64, (3,), convert=True)
        if vertices.device != dev:
            raise _lib.DudfError("vertices and faces must be on one device")
        if vertices.shape[0] != V:
            raise _lib.DudfError(f"vertices has {vertices.shape[0]} rows, n_vertices is {V}")
    ws, nbytes = _workspace(dev, "dudf_mesh_topology_workspace_bytes", F, err=-4)
    out_f = torch.empty(F, 3, dtype=torch.int64, device=dev)
    comp = torch.empty(F, dtype=torch.int64, device=dev)
    flip = torch.empty(F, dtype=torch.uint8, device=dev)
    nfaces = torch.empty(F, dtype=torch.int64, device=dev)
    area_q = torch.zeros(F, dtype=torch.int64, device=dev)
    counts = torch.zeros(len(MESH_TOPOLOGY_COUNTS), dtype=torch.int64, device=dev)
    _call("dudf_mesh_topology", _ptr(faces), F, V, _ptr(vertices), _ptr(out_f), _ptr(comp), _ptr(flip), _ptr(nfaces), _ptr(area_q),
          _ptr(counts), _ptr(ws), nbytes, dev=dev)
    return out_f, comp, flip, nfaces, area_q, dict(zip(MESH_TOPOLOGY_COUNTS, (int(v) for v in counts.tolist())))


def mesh_submesh(vertices, faces, keep):
    """The faces with keep != 0 in their order, the vertices they use in their order, faces re-indexed (`dudf_mesh_submesh_count` /
    `_emit`).  keep (F,) bool or uint8.  Returns (vertices (V',3) float64, faces (F',3) int64).  One host sync for the counts."""
    vertices, faces = _mesh(vertices, faces)
    dev = vertices.device
    V, F = vertices.shape[0], faces.shape[0]
    keep = _tensor(keep, "keep", torch.uint8, (), convert=True)
    if keep.shape[0] != F or keep.device != dev:
        raise _lib.DudfError(f"keep must be (F,) = ({F},) on the device of the mesh; got {tuple(keep.shape)} on {keep.device}")
    ws, nbytes = _workspace(dev, "dudf_mesh_submesh_workspace_bytes", V, F, err=-4)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    _call("dudf_mesh_submesh_count", V, _ptr(faces), F, _ptr(keep), _ptr(counts), _ptr(ws), nbytes, dev=dev)
    nv, nf = (int(v) for v in counts.tolist())
    out_v = torch.empty(nv, 3, dtype=torch.float64, device=dev); out_f = torch.empty(nf, 3, dtype=torch.int64, device=dev)
    if nv and nf:
        _call("dudf_mesh_submesh_emit", _ptr(vertices), V, _ptr(faces), F, _ptr(keep), _ptr(out_v), _ptr(out_f), _ptr(ws), nbytes, dev=dev)
    return out_v, out_f


MESH_SIMPLIFY_COUNTS = ("vertices", "faces", "cells", "collapsed", "duplicate", "invalid", "border_edges", "fallback")


def _simplify_count(vertices, faces, origin, cell, boundary_weight, tau, place):
    """`dudf_mesh_simplify_keys`, the stable sort of the corner keys (plumbing, as the Morton order of `mesh_index_build`) and
    `dudf_mesh_simplify_count`: (counts, what `_emit` needs).  One host sync: the counts."""
    vertices, faces = _mesh(vertices, faces)
    dev = vertices.device
    V, F = vertices.shape[0], faces.shape[0]
    org = _dbl(origin.tolist() if hasattr(origin, "tolist") else origin, 3, "origin")
    ws, nbytes = _workspace(dev, "dudf_mesh_simplify_workspace_bytes", V, F, err=-4)
    keys = torch.empty(3 * F, dtype=torch.int64, device=dev)
    head = (_ptr(vertices), V, _ptr(faces), F)
    _call("dudf_mesh_simplify_keys", *head, org, float(cell), _ptr(keys), _ptr(ws), nbytes, dev=dev)
    skeys, order = torch.sort(keys, stable=True)
    counts = torch.zeros(len(MESH_SIMPLIFY_COUNTS), dtype=torch.int64, device=dev)
    _call("dudf_mesh_simplify_count", *head, org, float(cell), float(boundary_weight), float(tau), _ptr(skeys), _ptr(order),
          int(bool(place)), _ptr(counts), _ptr(ws), nbytes, dev=dev)
    return dict(zip(MESH_SIMPLIFY_COUNTS, (int(v) for v in counts.tolist()))), (head, ws, nbytes, dev, (vertices, faces))


def mesh_simplify_count(vertices, faces, origin, cell):
    """The counts of `mesh_simplify` at lattice edge `cell` without the per-cell sums and placement (`fallback` is -1): what a search
    over the lattice for a face count asks.  One host sync."""
    return _simplify_count(vertices, faces, origin, cell, 0.0, 1e-3, False)[0]


def mesh_simplify(vertices, faces, origin, cell, boundary_weight=1.0, tau=1e-3, want_quadrics=False):
    """Quadric vertex clustering of a device mesh on the lattice of edge `cell` at `origin` (3 numbers) with border quadrics
    (`dudf_mesh_simplify_keys` / `_count` / `_emit`; the rules: DESIGN.md §3.6c).  Returns (vertices (V',3) float64, faces (F',3) int64,
    counts: a dict over MESH_SIMPLIFY_COUNTS) and with want_quadrics, per occupied cell in ascending key order, (quadrics (C,10), xhat
    (C,3), cell_keys (C,) int64, records (C,) int64, fell_back (C,) uint8).  One host sync: the counts, which size the outputs."""
    c, (head, ws, nbytes, dev, _mesh_alive) = _simplify_count(vertices, faces, origin, cell, boundary_weight, tau, True)
    nv, nf, nc = c["vertices"], c["faces"], c["cells"]
    out_v = torch.empty(max(nv, 1), 3, dtype=torch.float64, device=dev)              # emit wants the pointers even when nothing survives
    out_f = torch.empty(max(nf, 1), 3, dtype=torch.int64, device=dev)
    extra = ()
    if want_quadrics:
        extra = (torch.empty(nc, 10, dtype=torch.float64, device=dev), torch.empty(nc, 3, dtype=torch.float64, device=dev),
                 torch.empty(nc, dtype=torch.int64, device=dev), torch.empty(nc, dtype=torch.int64, device=dev),
                 torch.empty(nc, dtype=torch.uint8, device=dev))
    if nc:
        opt = tuple(_ptr(t) for t in extra) if extra else (None,) * 5
        _call("dudf_mesh_simplify_emit", *head, _ptr(out_v), _ptr(out_f), *opt, _ptr(ws), nbytes, dev=dev)
    return (out_v[:nv], out_f[:nf], c) + extra


def _w4(weights):
    w = list(weights) + [0.0] * (4 - len(weights))
    return (ctypes.c_double * 4)(*[float(v) for v in w])


def loss_forward(cfg, mode, theta, x, normals, sdf, n_global, weights, alpha, ws, n_hess=0, out=None):
    """n_hess > 0 (loss_s1 with a Hessian weight): the first n_hess points must be exactly the on-surface ones.
    `out`: a contiguous float32 tensor of 4 to receive the terms (no extra copy kernel in the training loop)."""
    _theta(cfg, theta, convert=False)
    n = x.shape[0]
    terms = out if out is not None else torch.empty(4, dtype=torch.float32, device=x.device)
    _call("dudf_loss_forward", ctypes.byref(cfg), mode, _ptr(theta), _ptr(x), _ptr(normals), _ptr(sdf), n, int(n_global),
          int(n_hess), _w4(weights), float(alpha), _ptr(terms), _ptr(ws.buf), ws.nbytes)
    return terms


def s2_forward_stats(cfg, theta, x, sdf, ws):
    _theta(cfg, theta, convert=False)
    stats = torch.empty(3, dtype=torch.float64, device=x.device)
    _call("dudf_s2_forward_stats", ctypes.byref(cfg), _ptr(theta), _ptr(x), _ptr(sdf), x.shape[0], _ptr(stats), _ptr(ws.buf),
          ws.nbytes)
    return stats


def s2_terms(stats, weights):
    terms = torch.empty(2, dtype=torch.float32, device=stats.device)
    _call("dudf_s2_terms", _ptr(stats), _w4(weights), _ptr(terms))
    return terms


def loss_backward(cfg, mode, theta, x, normals, sdf, n_global, weights, alpha, cot, stats, ws, dtheta=None,
                  accumulate=False, n_hess=0):
    if dtheta is None:
        dtheta = torch.empty_like(theta)
        accumulate = False
    _call("dudf_loss_backward", ctypes.byref(cfg), mode, _ptr(theta), _ptr(x), _ptr(normals), _ptr(sdf), x.shape[0], int(n_global),
          int(n_hess), _w4(weights), float(alpha), _ptr(cot), _ptr(stats), _ptr(dtheta), 1 if accumulate else 0, _ptr(ws.buf),
          ws.nbytes)
    return dtheta


def loss_backward_sweeps(cfg, mode, theta, normals, sdf, n_global, weights, alpha, cot, stats, ws, n_local, n_hess=0):
    """loss cotangents + adjoint sweeps; the weight gradients follow through `weight_gradient` (layer ranges)."""
    _theta(cfg, theta, convert=False)
    _call("dudf_loss_backward_sweeps", ctypes.byref(cfg), mode, _ptr(theta), _ptr(normals), _ptr(sdf), int(n_local), int(n_global),
          int(n_hess), _w4(weights), float(alpha), _ptr(cot), _ptr(stats), _ptr(ws.buf), ws.nbytes)


def layer_slices(cfg):
    """[(begin, end)] offsets into theta of layer 0 .. L (state_dict order: weight then bias)."""
    H, L = cfg.hidden, cfg.n_hidden_layers
    out, off = [(0, 4 * H)], 4 * H
    for _ in range(L - 1):
        out.append((off, off + H * H + H)); off += H * H + H
    out.append((off, off + H + 1))
    return out


def weight_gradient(cfg, n_local, have_g, layer_begin, layer_end, dtheta, ws, accumulate=False, n_hess=0):
    _call("dudf_weight_gradient", ctypes.byref(cfg), int(n_local), int(n_hess), 1 if have_g else 0, int(layer_begin),
          int(layer_end), _ptr(dtheta), 1 if accumulate else 0, _ptr(ws.buf), ws.nbytes)


def fields_forward(cfg, theta, x, ws):
    """(f (n,), df/dx (n,3)) with the training stash kept in ws (for fields_backward)."""
    _theta(cfg, theta, convert=False)
    n = x.shape[0]
    f = torch.empty(n, dtype=torch.float32, device=x.device)
    g = torch.empty(n, 3, dtype=torch.float32, device=x.device)
    _call("dudf_fields_forward", ctypes.byref(cfg), _ptr(theta), _ptr(x), n, _ptr(f), _ptr(g), _ptr(ws.buf), ws.nbytes)
    return f, g


def fields_backward(cfg, theta, x, ybar, gbar, ws, dtheta=None, accumulate=False):
    _theta(cfg, theta, convert=False)
    if dtheta is None:
        dtheta = torch.empty_like(theta)
        accumulate = False
    _call("dudf_fields_backward", ctypes.byref(cfg), _ptr(theta), _ptr(x), x.shape[0], _ptr(ybar), _ptr(gbar), _ptr(dtheta),
          1 if accumulate else 0, _ptr(ws.buf), ws.nbytes)
    return dtheta


def set_wgrad_max_workgroups(n):
    """Cap of the weight-gradient GEMM's grid (8..256 workgroups): TrainEngine leaves CUs to overlapping RCCL kernels."""
    set_option("wgrad_max_workgroups", int(n))


def adam_step(theta, dtheta, exp_avg, exp_avg_sq, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0):
    _call("dudf_adam_step", _ptr(theta), _ptr(dtheta), _ptr(exp_avg), _ptr(exp_avg_sq), theta.numel(), float(lr), float(beta1),
          float(beta2), float(eps), int(step), float(grad_scale))


def adam_schedule(lrs, first_step=1, beta1=0.9, beta2=0.999):
    """HOST table (len(lrs), 2) float32 of (lr / (1 - beta1^t), sqrt(1 - beta2^t)), t = first_step + i: the two step-dependent
    scalars `adam_step` derives on the host, for `adam_step_scheduled` (dudf_adam_schedule: host only, no GPU work)."""
    import numpy as np
    lr = np.ascontiguousarray(lrs, dtype=np.float64)
    out = np.empty((lr.size, 2), dtype=np.float32)
    _call("dudf_adam_schedule", lr.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), lr.size, int(first_step), float(beta1),
          float(beta2), ctypes.c_void_p(out.ctypes.data), stream=False)
    return out


def adam_step_scheduled(theta, dtheta, exp_avg, exp_avg_sq, sched, row, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0):
    """`adam_step` with (lr, step) replaced by row `row[0]` (device int64, NOT advanced here) of the device table `sched`
    (`adam_schedule(...)` uploaded): graph-replayable."""
    assert sched.dtype == torch.float32 and sched.is_contiguous() and sched.shape[-1] == 2 and row.dtype == torch.int64
    _call("dudf_adam_step_scheduled", _ptr(theta), _ptr(dtheta), _ptr(exp_avg), _ptr(exp_avg_sq), theta.numel(), float(beta1),
          float(beta2), float(eps), _ptr(sched), sched.shape[0], _ptr(row), float(grad_scale))


def read_stash(cfg, which, layer, n, ws, channel=0):
    """Diagnostic: (n,H) copy of one stashed quantity of hidden layer `layer` (channel 1..3 = tangent d/dx_k,
    Hessian-path points only)."""
    idx = {"s": 0, "c": 1, "q": 2, "e": 3, "A": 4, "zbar": 5, "r": 6, "zs": 7}[which]
    out = torch.empty(n, cfg.hidden, dtype=torch.float32, device=ws.buf.device)
    _call("dudf_debug_read_stash", ctypes.byref(cfg), idx, layer, channel, n, ws.n_hess, _ptr(out), _ptr(ws.buf), ws.nbytes)
    return out


def debug_eigh3(H):
    """Diagnostic: (lam (k,3) ascending, V (k,3,3) with V[m,i,j] = component i of v_j) of the device's 3x3 eigensolver on the LOWER
    triangles of H (k,3,3) float64 — the routine of the loss kernels, the CAP-UDF frame, the curvature and the cloud normals."""
    H = _tensor(H, "H", torch.float64, (3, 3))
    k = H.shape[0]
    lam = torch.empty(k, 3, dtype=torch.float64, device=H.device)
    V = torch.empty(k, 3, 3, dtype=torch.float64, device=H.device)
    _call("dudf_debug_eigh3", _ptr(H), k, _ptr(lam), _ptr(V), dev=H.device)
    return lam, V


def debug_loss_stage(cfg, mode, y, g, h, normals, sdf, n_global, weights, alpha, cot, ws, stats=None):
    """Diagnostic: the loss kernels alone on planted fields — y (n), g (n,3), h (n_hess,3,3) or None, normals (n,3), sdf (n), cot (4),
    all float32 on the GPU; ws = workspace_for(cfg, n, device, n_hess); stats (3 float64, loss_s2): the statistics the backward
    uses instead of the batch's own.  No sweep runs.  Returns a dict: terms (4), stats (3 float64, loss_s2) or None, ybar (n), gbar
    (n,3), hbar (n_hess,3,3) or None, pad_nonzero (the count of floats-owed-a-zero columns that are not, include/dudf_hip.h)."""
    n, n_hess, dev = y.shape[0], ws.n_hess, y.device
    y = _tensor(y, "y", torch.float32, ())
    g = _tensor(g, "g", torch.float32, (3,))
    normals = _tensor(normals, "normals", torch.float32, (3,))
    sdf = _tensor(sdf, "sdf", torch.float32, ())
    cot = _tensor(cot, "cot", torch.float32, ())
    if n != ws.n or (h.shape[0] if h is not None else 0) != n_hess or g.shape[0] != n or normals.shape[0] != n or sdf.shape[0] != n \
            or cot.shape[0] != 4:
        raise _lib.DudfError(f"debug_loss_stage: {n} points with {0 if h is None else h.shape[0]} Hessians on a workspace for "
                             f"({ws.n}, {ws.n_hess})")
    if h is not None:
        h = _tensor(h, "h", torch.float32, (3, 3))
    if stats is not None:
        stats = _tensor(stats, "stats", torch.float64, ())
    out = {"terms": torch.empty(4, dtype=torch.float32, device=dev),
           "stats": torch.empty(3, dtype=torch.float64, device=dev) if mode == LOSS_S2 else None,
           "ybar": torch.empty(n, dtype=torch.float32, device=dev), "gbar": torch.empty(n, 3, dtype=torch.float32, device=dev),
           "hbar": torch.empty(n_hess, 3, 3, dtype=torch.float32, device=dev) if n_hess else None}
    pad = torch.empty(1, dtype=torch.int32, device=dev)
    _call("dudf_debug_loss_stage", ctypes.byref(cfg), mode, n, n_hess, _ptr(y), _ptr(g), _ptr(h), _ptr(normals), _ptr(sdf),
          int(n_global), _w4(weights), float(alpha), _ptr(cot), _ptr(stats), _ptr(out["terms"]), _ptr(out["stats"]), _ptr(out["ybar"]),
          _ptr(out["gbar"]), _ptr(out["hbar"]), _ptr(pad), _ptr(ws.buf), ws.nbytes, dev=dev)
    out["pad_nonzero"] = int(pad.item())
    return out


# ---- sphere-traced images (reference generate_st.py, src/render_st.py:67-245) ---------------------------------------------------
SHADE_MODELS = {"blinn-phong": 0, "ward": 1}


def _dbl(values, n, what):
    vals = [float(v) for v in values]
    if len(vals) != n:
        raise _lib.DudfError(f"{what} takes {n} numbers; got {len(vals)}")
    return (ctypes.c_double * n)(*vals)


def render_setup_rays(width, height, fov, noise, rotation, camera_position, planes, device):
    """`dudf_render_setup_rays`: rays (m,3), t0 (m,3) float64 and mask (m,) uint8 on `device` for the width * height pixels of
    `get_pixels_camera(width, height, fov, noise)` — reference generate_st.py:41-101.  rotation: the 3x3 of :49-61 (host)."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.DudfError(f"render_setup_rays: device must be a GPU (got {dev}); the HIP path has no CPU fallback")
    m = int(width) * int(height)
    rays = torch.empty(m, 3, dtype=torch.float64, device=dev); t0 = torch.empty(m, 3, dtype=torch.float64, device=dev)
    mask = torch.empty(m, dtype=torch.uint8, device=dev)
    rot = _dbl([v for row in rotation for v in row], 9, "rotation")
    _call("dudf_render_setup_rays", int(width), int(height), float(fov), float(noise), rot,
          _dbl(camera_position, 3, "camera_position"), _dbl(planes, 6, "planes"), _ptr(rays), _ptr(t0), _ptr(mask), dev=dev)
    return rays, t0, mask


def render_gather(hits, t0, rays=None):
    """`t0[hits]`, `rays[hits]` and the ray index of every gathered row (`dudf_render_gather`).  Returns (pos (k,3), rays (k,3) or
    None, rows (k,) int32, k); k is the ONE host read of a pass."""
    hits = _tensor(hits, "render_gather: hits", torch.uint8, ())
    t0 = _tensor(t0, "render_gather: t0", torch.float64, (3,))
    m, dev = hits.shape[0], hits.device
    if rays is not None:
        rays = _tensor(rays, "render_gather: rays", torch.float64, (3,))
    if t0.shape[0] != m or (rays is not None and rays.shape[0] != m):
        raise _lib.DudfError("render_gather: row counts of hits, t0 and rays differ")
    pos = torch.empty(m, 3, dtype=torch.float64, device=dev)
    hr = torch.empty(m, 3, dtype=torch.float64, device=dev) if rays is not None else None
    rows = torch.empty(m, dtype=torch.int32, device=dev)
    counter = torch.empty(4, dtype=torch.int64, device=dev)
    ws, nbytes = _workspace(dev, "dudf_pointcloud_append_workspace_bytes", m)
    _call("dudf_render_gather", _ptr(hits), m, _ptr(t0), _ptr(rays), _ptr(pos), _ptr(hr), _ptr(rows), _ptr(counter), _ptr(ws),
          nbytes, dev=dev)
    k = int(counter[1].item())
    return pos[:k], (hr[:k] if hr is not None else None), rows[:k], k


def render_orient(hit_rays, frame_v=None, grad=None, mean=None, want_pc=False):
    """Normals of k hits (`dudf_render_orient`, reference src/render_st.py:80-83, :101-108): from the eigen-frame `frame_v` (k,3,3),
    oriented against the rays (`mean` (k,) float32 is multiplied in place by the same alignment), or from `grad` (k,3) ('siren').
    Returns (normals (k,3) float64, pc1, pc2 (k,3) float64 or None)."""
    src = frame_v if frame_v is not None else grad
    if src is None or (frame_v is not None and grad is not None):
        raise _lib.DudfError("render_orient: exactly one of frame_v / grad")
    src = _tensor(src, "render_orient: frame_v / grad", torch.float32, convert=True)
    k, dev = src.shape[0], src.device
    if frame_v is not None:
        hit_rays = _tensor(hit_rays, "render_orient: hit_rays", torch.float64, (3,))
        if tuple(src.shape) != (k, 3, 3) or hit_rays.shape[0] != k:
            raise _lib.DudfError(f"render_orient: frame_v must be (k,3,3) with k rays; got {tuple(src.shape)}, {tuple(hit_rays.shape)}")
        if mean is not None and _tensor(mean, "render_orient: mean", torch.float32).numel() != k:
            raise _lib.DudfError("render_orient: mean must be a float32 vector of k")
    elif tuple(src.shape) != (k, 3):
        raise _lib.DudfError(f"render_orient: grad must be (k,3); got {tuple(src.shape)}")
    normals = torch.empty(k, 3, dtype=torch.float64, device=dev)
    pc1 = torch.empty(k, 3, dtype=torch.float64, device=dev) if want_pc and frame_v is not None else None
    pc2 = torch.empty(k, 3, dtype=torch.float64, device=dev) if want_pc and frame_v is not None else None
    _call("dudf_render_orient", _ptr(src) if frame_v is not None else None, _ptr(src) if frame_v is None else None,
          _ptr(hit_rays) if frame_v is not None else None, k, _ptr(normals), _ptr(pc1), _ptr(pc2),
          _ptr(mean) if frame_v is not None else None, dev=dev)
    return normals, pc1, pc2


def render_percentile_bounds(curvatures, q_low, q_high):
    """(2,) float32 on the device: `np.percentile(curvatures, q)` for the two q of reference src/render_st.py:111, bit for bit what
    numpy 2.x returns for a float32 array and python numbers q (default 'linear' method).  That numpy keeps the array's dtype
    throughout: q is rounded to float32 and divided by float32(100); the virtual index is float32(k - 1) times that; the weight
    is the index minus its floor; and its _lerp is a + (b - a) t for t < 0.5, b - (b - a) (1 - t) otherwise, every product,
    sum and 1 - t rounded to float32.  An index at or past k - 1 takes the largest value, a NaN anywhere gives NaN.  The index
    and the weight depend on k and q alone and are formed on the host; torch.sort is the plumbing; nothing is read back."""
    f32 = np.float32
    k = curvatures.numel()
    s = torch.sort(curvatures.reshape(-1).float()).values            # NaN sorts last, as in numpy
    out = []
    for q in (q_low, q_high):
        virtual = f32(k - 1) * (f32(q) / f32(100))
        if virtual >= f32(k - 1):
            r = s[k - 1]
        else:
            lo = int(np.floor(virtual))
            t = virtual - f32(lo)
            a, b = s[lo], s[lo + 1]
            diff = b - a
            r = a + diff * float(t) if t < f32(0.5) else b - diff * float(f32(1) - t)
        out.append(torch.where(torch.isnan(s[k - 1]), s[k - 1], r))
    return torch.stack(out)


def render_colormap(curvatures, bounds, lut):
    """(k,3) float64 colours of k float32 curvatures (`dudf_render_colormap`, reference src/render_st.py:111-114)."""
    curvatures = _tensor(curvatures, "render_colormap: curvatures", torch.float32, convert=True).reshape(-1)
    bounds = _tensor(bounds, "render_colormap: bounds", torch.float32, convert=True)
    lut = _tensor(lut, "render_colormap: lut", torch.float64, (3,))
    if tuple(lut.shape) != (256, 3) or bounds.numel() != 2:
        raise _lib.DudfError(f"render_colormap: lut must be (256,3) and bounds 2 floats; got {tuple(lut.shape)}, {bounds.numel()}")
    k = curvatures.shape[0]
    out = torch.empty(k, 3, dtype=torch.float64, device=curvatures.device)
    _call("dudf_render_colormap", _ptr(curvatures), k, _ptr(bounds), _ptr(lut), _ptr(out), dev=curvatures.device)
    return out


def render_shade(model, hits, rows, hit_pos, normals, accumulator, light_position, camera_position=None, shininess=0.0, alpha1=0.0,
                 alpha2=0.0, pc1=None, pc2=None, color_map=None):
    """`dudf_render_shade`: accumulator (m,3) float64 += phong / ward colours of the k hits at their image rows, += 1 elsewhere
    (reference src/render_st.py:174-245)."""
    if model not in SHADE_MODELS:
        raise _lib.DudfError(f"reflection_method must be one of {sorted(SHADE_MODELS)}; got {model!r}")
    hits = _tensor(hits, "render_shade: hits", torch.uint8, ())
    accumulator = _tensor(accumulator, "render_shade: accumulator", torch.float64, (3,))
    m, k = hits.shape[0], rows.shape[0]
    if accumulator.shape[0] != m:
        raise _lib.DudfError("render_shade: accumulator must have one row per ray")
    _tensor(rows, "render_shade: rows", torch.int32)
    arrs = [("hit_pos", hit_pos), ("normals", normals)]
    if model == "ward":
        if pc1 is None or pc2 is None or camera_position is None:
            raise _lib.DudfError("render_shade: ward takes pc1, pc2 and the camera position")
        arrs += [("pc1", pc1), ("pc2", pc2)]
    if color_map is not None:
        arrs.append(("color_map", color_map))
    for name, t in arrs:
        if _tensor(t, f"render_shade: {name}", torch.float64, (3,)).shape[0] != k:
            raise _lib.DudfError(f"render_shade: {name} has {t.shape[0]} rows for {k} hits")
    _call("dudf_render_shade", SHADE_MODELS[model], _ptr(hits), m, _ptr(rows), k, _ptr(hit_pos), _ptr(normals), _ptr(pc1),
          _ptr(pc2), _ptr(color_map), _dbl(light_position, 3, "light_position"),
          _dbl(camera_position, 3, "camera_position") if camera_position is not None else None, float(shininess), float(alpha1),
          float(alpha2), _ptr(accumulator), dev=hits.device)


def render_finish(accumulator, sample_rate):
    """uint8 tensor of accumulator's shape: `(colores / sample_rate * 255).astype(np.uint8)` (reference generate_st.py:139)."""
    _tensor(accumulator, "render_finish: accumulator", torch.float64)
    out = torch.empty(accumulator.shape, dtype=torch.uint8, device=accumulator.device)
    _call("dudf_render_finish", _ptr(accumulator), accumulator.numel(), float(sample_rate), _ptr(out), dev=accumulator.device)
    return out


def render_traced(cfg, theta, rays, t0, mask, network_config, rendering_config, lut, accumulator):
    """Steps 2-8 of a pass on device arrays (reference src/render_st.py:67-133 `create_projectional_image`): march, descend, gather,
    query the hits only, orient, percentiles + colour map, shade into `accumulator` (m,3) float64 (+=).  t0 and mask are updated in
    place.  Returns (hits (m,) uint8, k).  The hit count is the only value read back; 0 hits raise the reference's ValueError."""
    nc, rc_ = network_config, rendering_config
    gt_mode = nc['gt_mode']
    plot = rc_.get('plot_curvatures', 'none')
    method = rc_.get('reflection_method', 'blinn-phong')
    if gt_mode != 'siren':
        if method not in SHADE_MODELS:
            raise _lib.DudfError(f"reflection_method must be one of {sorted(SHADE_MODELS)}; got {method!r}")
        if plot in ('mean', 'gaussian') and lut is None:
            raise _lib.DudfError("plotting curvatures needs the (256,3) colour table (matplotlib's RdYlBu in the reference); none was given")
    with torch.cuda.device(t0.device):
        hits, _ = trace_rays(cfg, theta, rays, t0, mask, gt_mode, nc['alpha'], rc_['surface_threshold'], rc_['max_iterations'])
        if rc_.get('gd_steps', 0) > 0:
            descend_rays(cfg, theta, t0, hits, gt_mode, nc['alpha'], rc_['gd_steps'])
        pos, hit_rays, rows, k = render_gather(hits, t0, rays)
        if k == 0:
            raise ValueError(f"Ray tracing did not converge in {rc_['max_iterations']} iterations to any point at distance "
                             f"{rc_['surface_threshold']} or lower from surface.")
        x = pos.float()                                      # the network sees float32 copies (reference src/render_st.py:25)
        if gt_mode == 'siren':
            _, g = query(cfg, theta, x)
            normals, _, _ = render_orient(None, grad=g)
            render_shade("blinn-phong", hits, rows, pos, normals, accumulator, rc_['light_position'], shininess=rc_['shininess'])
            return hits, k
        curv = None
        if plot in ('mean', 'gaussian'):                     # normals and mean curvature from the SAME eigen-frame: one sign
            _, V, mean, gauss, _ = query_curvature(cfg, theta, x, want_shape=(plot == 'gaussian'))
            curv = mean if plot == 'mean' else gauss
        else:
            V = query_frame(cfg, theta, x)[4]
        normals, pc1, pc2 = render_orient(hit_rays, frame_v=V, mean=curv if plot == 'mean' else None, want_pc=(method == 'ward'))
        colors = None
        if curv is not None:
            bounds = render_percentile_bounds(curv, rc_['curv_low_bound'], rc_['curv_high_bound'])
            colors = render_colormap(curv, bounds, lut)
        if method == 'ward':
            render_shade("ward", hits, rows, pos, normals, accumulator, rc_['light_position'], rc_['camera_position'],
                         alpha1=rc_['alpha1'], alpha2=rc_['alpha2'], pc1=pc1, pc2=pc2, color_map=colors)
        else:
            render_shade("blinn-phong", hits, rows, pos, normals, accumulator, rc_['light_position'], shininess=rc_['shininess'],
                         color_map=colors)
    return hits, k


def render_pass(cfg, theta, noise, rotation, camera_position, network_config, rendering_config, lut, accumulator):
    """One jittered pass of reference generate_st.py:41-135 on the device: ray set-up, then `render_traced`.  accumulator
    (height * width, 3) float64 CUDA tensor, += like `colores`.  Returns the hit count."""
    rc_ = rendering_config
    # the reference hands (height, width) to get_pixels_camera(width, height, ...) (:42); kept
    rays, t0, mask = render_setup_rays(rc_['height'], rc_['width'], rc_['fov'], noise, rotation, camera_position,
                                       rc_.get('planes', [1, -1, 1, -1, 1, -1]), accumulator.device)
    return render_traced(cfg, theta, rays, t0, mask, network_config, rendering_config, lut, accumulator)[1]


# ---- Chamfer distance / normal consistency (reference cuantitative.py:10-19, :99-100; csrc/dudf_chamfer.hip) -------------------
def nearest_points(x, y, norm=2, want_dist=True, want_idx=True):
    """For every row of x (n,3) the nearest row of y (m,3) — `knn_points(x, y, norm=norm, K=1)` of pytorch3d: (dist (n,) float32,
    idx (n,) int64).  norm 2: SQUARED Euclidean distance; norm 1: L1 distance.  Smallest index among ties; bit-reproducible."""
    x = _tensor(x, "nearest_points: x", torch.float32, (3,), convert=True); y = _tensor(y, "nearest_points: y", torch.float32, (3,), convert=True)
    if y.device != x.device:
        raise _lib.DudfError("nearest_points: x and y live on different devices")
    n, m, dev = x.shape[0], y.shape[0], x.device
    dist = torch.empty(n, dtype=torch.float32, device=dev) if want_dist else None
    idx = torch.empty(n, dtype=torch.int64, device=dev) if want_idx else None
    ws, nbytes = _workspace(dev, "dudf_nearest_workspace_bytes", n)
    _call("dudf_nearest_points", _ptr(x), n, _ptr(y), m, int(norm), _ptr(dist), _ptr(idx), _ptr(ws), nbytes, dev=dev)
    return dist, idx


def chamfer_terms(dist, idx, x_normals=None, y_normals=None, out=None):
    """(2,) float64 CUDA tensor: sum of dist and sum of 1 - |cos(x_normals[p], y_normals[idx[p]])| (the second stays 0 without
    normals).  Double accumulation in a fixed order: bit-reproducible."""
    _tensor(dist, "chamfer_terms: dist", torch.float32, ())
    n, dev, m = dist.shape[0], dist.device, 0
    if (x_normals is None) != (y_normals is None):
        raise _lib.DudfError("chamfer_terms: x_normals and y_normals come together")
    if x_normals is not None:
        x_normals = _tensor(x_normals, "chamfer_terms: x_normals", torch.float32, (3,), convert=True)
        y_normals = _tensor(y_normals, "chamfer_terms: y_normals", torch.float32, (3,), convert=True)
        if _tensor(idx, "chamfer_terms: idx", torch.int64, ()).shape != dist.shape:
            raise _lib.DudfError("chamfer_terms: idx must have one entry per distance")
        if x_normals.shape[0] != n:
            raise _lib.DudfError("chamfer_terms: x_normals must have one row per distance")
        m = y_normals.shape[0]
    if out is None:
        out = torch.zeros(2, dtype=torch.float64, device=dev)
    elif _tensor(out, "chamfer_terms: out", torch.float64).numel() != 2:
        raise _lib.DudfError("chamfer_terms: out must be a float64 tensor of 2")
    ws, nbytes = _workspace(dev, "dudf_chamfer_terms_workspace_bytes", n)
    _call("dudf_chamfer_terms", _ptr(dist), _ptr(idx) if x_normals is not None else _ptr(None), n, _ptr(x_normals),
          _ptr(y_normals), m, _ptr(out), _ptr(ws), nbytes, dev=dev)
    return out


def vertex_normals(vertices, faces):
    """(V,3) float32 area-weighted unit vertex normals of a triangle mesh — open3d's `compute_vertex_normals(normalized=True)`
    (reference cuantitative.py:99-100).  vertices (V,3) float64 and faces (F,3) int64 CUDA tensors (other dtypes are converted)."""
    vertices = _tensor(vertices, "vertex_normals: vertices", torch.float64, (3,), convert=True)
    if torch.is_tensor(faces) and faces.numel() == 0:
        faces = faces.reshape(0, 3)
    faces = _tensor(faces, "vertex_normals: faces", torch.int64, (3,), convert=True)
    if faces.device != vertices.device:
        raise _lib.DudfError("vertex_normals: vertices and faces live on different devices")
    nv, nf, dev = vertices.shape[0], faces.shape[0], vertices.device
    out = torch.empty(nv, 3, dtype=torch.float32, device=dev)
    ws, nbytes = _workspace(dev, "dudf_vertex_normals_workspace_bytes", nv)
    _call("dudf_vertex_normals", _ptr(vertices), nv, _ptr(faces), nf, _ptr(out), _ptr(ws), nbytes, dev=dev)
    return out


# ---- surface samples and threshold statistics (csrc/dudf_surfsample.hip) -----------------------------------------
STATS_MAX_K = 16


def mesh_sample_surface(vertices, faces, n, seed=123, start=0, uniforms=None, want_points=True, want_normals=True, want_face=False,
                        want_face_normals=False, want_area=False):
    """`dudf_mesh_sample_surface`: (points (n,3) float32, normals (n,3) float32, face (n,) int64, face_normals (F,3) float32, area
    float64 CUDA tensor of 1) — None for what was not asked for — of the samples start .. start + n - 1 of the mesh vertices (V,3)
    float64, faces (F,3) int64 (CUDA tensors; other dtypes are converted).  uniforms (n,3) float64: the three numbers of every
    sample instead of the generator's, each in [0, 1) (checked by the caller).  ValueError for a non-finite vertex or a face index
    out of range, DudfError for a mesh without faces or without area."""
    vertices = _tensor(vertices, "mesh_sample_surface: vertices", torch.float64, (3,), convert=True)
    if torch.is_tensor(faces) and faces.numel() == 0:
        faces = faces.reshape(0, 3)
    faces = _tensor(faces, "mesh_sample_surface: faces", torch.int64, (3,), convert=True)
    if faces.device != vertices.device:
        raise _lib.DudfError("mesh_sample_surface: vertices and faces live on different devices")
    V, F, dev, n, start = vertices.shape[0], faces.shape[0], vertices.device, int(n), int(start)
    if n < 0 or start < 0:
        raise _lib.DudfError(f"mesh_sample_surface: n and start must not be negative; got {n}, {start}")
    if F == 0 or V == 0:
        raise _lib.DudfError("mesh_sample_surface: a mesh without faces has no surface (DUDF_E_BADCFG)")
    if uniforms is not None:
        uniforms = _tensor(uniforms, "mesh_sample_surface: uniforms", torch.float64, (3,))
        if uniforms.shape[0] != n or uniforms.device != dev:
            raise _lib.DudfError("mesh_sample_surface: uniforms must be (n,3) on the device of the mesh")
    want_points = want_points or n > 0
    points = torch.empty(n, 3, dtype=torch.float32, device=dev) if want_points else None
    normals = torch.empty(n, 3, dtype=torch.float32, device=dev) if want_normals else None
    face = torch.empty(n, dtype=torch.int64, device=dev) if want_face else None
    face_normals = torch.empty(F, 3, dtype=torch.float32, device=dev) if want_face_normals else None
    area = torch.empty(1, dtype=torch.float64, device=dev) if want_area else None
    ws, nbytes = _workspace(dev, "dudf_mesh_sample_surface_workspace", F, err=-4)
    fn = getattr(_lib.load(), "dudf_mesh_sample_surface")
    with torch.cuda.device(dev):
        rc = fn(_ptr(vertices), V, _ptr(faces), F, start, n, int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(uniforms), _ptr(points), _ptr(normals),
                _ptr(face), _ptr(face_normals), _ptr(area), _ptr(ws), nbytes, _stream())
    if rc == -3:
        raise ValueError("mesh_sample_surface: the mesh has a NaN or infinite vertex, or a face refers to a vertex that does not exist")
    if rc == -1:
        raise _lib.DudfError("mesh_sample_surface: every face of the mesh is degenerate: there is no area to sample (DUDF_E_BADCFG)")
    _lib.check(rc, "dudf_mesh_sample_surface")
    return points, normals, face, face_normals, area


def distance_stats(dist, thresholds=()):
    """`dudf_distance_stats` of dist (n,) float32 (a CUDA tensor): (counts (K + 1,) int64 — rows with d <= tau_k, inclusive and
    compared in double, then the NaN rows —, max (1,) float32, sums (2,) float64: sum d and sum d*d over the rows that are not NaN),
    CUDA tensors.  Up to 16 thresholds.  Bit-reproducible."""
    _tensor(dist, "distance_stats: dist", torch.float32, ())
    taus = [float(t) for t in thresholds]
    K, n, dev = len(taus), dist.shape[0], dist.device
    if K > STATS_MAX_K:
        _lib.check(-4, f"dudf_distance_stats ({K} thresholds; at most {STATS_MAX_K})")
    counts = torch.empty(K + 1, dtype=torch.int64, device=dev)
    mx = torch.empty(1, dtype=torch.float32, device=dev)
    sums = torch.empty(2, dtype=torch.float64, device=dev)
    ws, nbytes = _workspace(dev, "dudf_distance_stats_workspace_bytes", n)
    _call("dudf_distance_stats", _ptr(dist), n, (ctypes.c_double * max(K, 1))(*taus), K, _ptr(counts), _ptr(mx), _ptr(sums), _ptr(ws),
          nbytes, dev=dev)
    return counts, mx, sums


# ---- K nearest neighbours and normal orientation (reference generate_pc.py:40; csrc/dudf_orient.hip) ----------------------------
KNN_MAX_K = 16


def knn_points(x, y, K=1, exclude_self=False, brute=False, want_dist=True, want_idx=True):
    """For every row of x (n,3) its K nearest rows of y (m,3) by squared Euclidean distance — `knn_points(x, y, K=K)` of pytorch3d:
    (dist (n,K) float32, idx (n,K) int64), each row ascending by (distance, index); a row with fewer than K candidates is padded with
    +inf / -1.  exclude_self (for x is y): row i never returns i.  brute=True scans all of y instead of walking the cell list built
    over it (the same bits).  Bit-reproducible; K = 1 equals `nearest_points`."""
    x = _tensor(x, "knn_points: x", torch.float32, (3,), convert=True); y = _tensor(y, "knn_points: y", torch.float32, (3,), convert=True)
    if y.device != x.device:
        raise _lib.DudfError("knn_points: x and y live on different devices")
    K, mode = int(K), 1 if brute else 0
    n, m, dev = x.shape[0], y.shape[0], x.device
    dist = torch.empty(n, K, dtype=torch.float32, device=dev) if want_dist and K > 0 else None
    idx = torch.empty(n, K, dtype=torch.int64, device=dev) if want_idx and K > 0 else None
    ws, nbytes = _workspace(dev, "dudf_knn_workspace_bytes", n, m, K, mode, err=-4)
    _call("dudf_knn_points", _ptr(x), n, _ptr(y), m, K, int(bool(exclude_self)), mode, _ptr(dist), _ptr(idx), _ptr(ws), nbytes, dev=dev)
    return dist, idx


def knn_grid_build(y):
    """The cell list `knn_points` builds over y (m,3) before it searches, alone (for timing); returns the workspace that holds it."""
    y = _tensor(y, "knn_grid_build: y", torch.float32, (3,), convert=True)
    ws, nbytes = _workspace(y.device, "dudf_knn_workspace_bytes", 0, y.shape[0], 1, 0, err=-4)
    _call("dudf_knn_grid_build", _ptr(y), y.shape[0], _ptr(ws), nbytes, dev=y.device)
    return ws


def orient_normals(points, normals, knn_idx, out=None):
    """Consistent signs for the normals (n,3) of the cloud points (n,3) over the graph knn_idx (n,K) int64 (`knn_points(points, points,
    K, exclude_self=True)`; entries outside [0, n) or equal to their row are no edges) — DESIGN.md §3.7.  Returns (normals (n,3)
    float32: the input or its negation, written to `out` if given — which may be `normals` itself —, flip (n,) uint8, component (n,)
    int64, counts (2,) int64 on the device: components and forest edges, stats: {"rounds", "launches"}).  Synchronises the stream
    once per round.  Byte-reproducible."""
    points = _tensor(points, "orient_normals: points", torch.float32, (3,), convert=True)
    normals = _tensor(normals, "orient_normals: normals", torch.float32, (3,), convert=True)
    if not torch.is_tensor(knn_idx) or knn_idx.dim() != 2:
        raise _lib.DudfError("orient_normals: knn_idx must be an (n, K) tensor")
    knn_idx = _tensor(knn_idx, "orient_normals: knn_idx", torch.int64, (knn_idx.shape[1],), convert=True)
    n, K, dev = points.shape[0], knn_idx.shape[1], points.device
    if normals.shape[0] != n or knn_idx.shape[0] != n or normals.device != dev or knn_idx.device != dev:
        raise _lib.DudfError("orient_normals: points, normals and knn_idx must have one row per point and live on one device")
    if out is None:
        out = torch.empty_like(normals)
    elif _tensor(out, "orient_normals: out", torch.float32, (3,)).shape != normals.shape or out.device != dev:
        raise _lib.DudfError("orient_normals: out must have the shape and device of normals")
    flip = torch.empty(n, dtype=torch.uint8, device=dev)
    comp = torch.empty(n, dtype=torch.int64, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    stats = (ctypes.c_int64 * 2)()
    ws, nbytes = _workspace(dev, "dudf_orient_workspace_bytes", n, K, err=-4)
    _call("dudf_orient_normals", _ptr(points), _ptr(normals), _ptr(knn_idx), n, K, _ptr(out), _ptr(flip), _ptr(comp), _ptr(counts), stats,
          _ptr(ws), nbytes, dev=dev)
    return out, flip, comp, counts, {"rounds": int(stats[0]), "launches": int(stats[1])}


# ---- raw scans: estimated normals and the statistical outlier test (open3d's stand-ins; csrc/dudf_cloudprep.hip) --------------------
def estimate_normals(points, knn_idx, include_self=True, want_info=False):
    """Unoriented normals (n,3) float32 of the cloud points (n,3) from the graph knn_idx (n,K) int64 (`knn_points(points, points, K,
    exclude_self=True)`): the eigenvector of the smallest eigenvalue of the fp64 covariance of every neighbourhood — the point itself
    with include_self, then its row's slots; fewer than 3 points, coincident points or a non-finite coordinate give (0, 0, 1)
    (DESIGN.md §3.8).  Returns (normals, eigenvalues (n,3) float64 ascending, counts (n,) int32); the last two are None without
    want_info.  Byte-reproducible."""
    points = _tensor(points, "estimate_normals: points", torch.float32, (3,), convert=True)
    if not torch.is_tensor(knn_idx) or knn_idx.dim() != 2:
        raise _lib.DudfError("estimate_normals: knn_idx must be an (n, K) tensor")
    knn_idx = _tensor(knn_idx, "estimate_normals: knn_idx", torch.int64, (knn_idx.shape[1],), convert=True)
    n, K, dev = points.shape[0], knn_idx.shape[1], points.device
    if knn_idx.shape[0] != n or knn_idx.device != dev:
        raise _lib.DudfError("estimate_normals: points and knn_idx must have one row per point and live on one device")
    out = torch.empty(n, 3, dtype=torch.float32, device=dev)
    eig = torch.empty(n, 3, dtype=torch.float64, device=dev) if want_info else None
    cnt = torch.empty(n, dtype=torch.int32, device=dev) if want_info else None
    ws, nbytes = _workspace(dev, "dudf_estimate_normals_workspace_bytes", n, K, err=-4)
    _call("dudf_estimate_normals", _ptr(points), _ptr(knn_idx), n, K, int(bool(include_self)), _ptr(out), _ptr(eig), _ptr(cnt), _ptr(ws),
          nbytes, dev=dev)
    return out, eig, cnt


def cloud_outliers(knn_dist, std_ratio=2.0):
    """The statistical outlier test on knn_dist (n,K) float32, the squared distances of `knn_points(points, points, K,
    exclude_self=True)`: (mean_dist (n,) float64 = the mean distance of every row to its finite neighbours, keep (n,) uint8 =
    mean_dist <= mu + std_ratio * sigma, stats (3,) float64 on the device = mu, sigma, threshold over the finite rows, kept_idx (n,)
    int64 whose head holds the kept rows in ascending order, counts (1,) int64 on the device = how many) — DESIGN.md §3.8.  Nothing is
    read back.  Byte-reproducible."""
    if not torch.is_tensor(knn_dist) or knn_dist.dim() != 2:
        raise _lib.DudfError("cloud_outliers: knn_dist must be an (n, K) tensor")
    knn_dist = _tensor(knn_dist, "cloud_outliers: knn_dist", torch.float32, (knn_dist.shape[1],), convert=True)
    n, K, dev = knn_dist.shape[0], knn_dist.shape[1], knn_dist.device
    mean = torch.empty(n, dtype=torch.float64, device=dev)
    keep = torch.empty(n, dtype=torch.uint8, device=dev)
    stats = torch.full((3,), float("nan"), dtype=torch.float64, device=dev)
    kept = torch.empty(n, dtype=torch.int64, device=dev)
    counts = torch.zeros(1, dtype=torch.int64, device=dev)
    ws, nbytes = _workspace(dev, "dudf_cloud_outliers_workspace_bytes", n, K, err=-4)
    _call("dudf_cloud_outliers", _ptr(knn_dist), n, K, float(std_ratio), _ptr(mean), _ptr(keep), _ptr(stats), _ptr(kept), _ptr(counts),
          _ptr(ws), nbytes, dev=dev)
    return mean, keep, stats, kept, counts


# ---- distance to a triangle mesh (reference generate_df.py:108-110, open3d RaycastingScene; csrc/dudf_bvh.hip, csrc/dudf_meshdist.hip) --
MESH_INDEX_FLAGS_OFFSET, MESH_FLAG_NONFINITE, MESH_FLAG_BAD_ORDER = 24, 1, 2       # include/dudf_hip.h


def _index_build(what, prefix, rows, width, order, nouns):
    """The index of `rows` (n, width) float32 through the entry points `prefix`_index_bytes / _morton_codes / _index_build: Morton
    codes on the device, a stable `torch.sort` (or the caller's `order`), then the boxes level by level; one host read at the end (the
    flag word).  nouns = (the shape, one row, the rows, its size letter, the argument's name), for the messages."""
    shape, row, plural, letter, arg = nouns
    rows = _tensor(rows, f"{what}: {arg}", torch.float32, (width,), convert=True)
    n, dev = rows.shape[0], rows.device
    if n == 0:
        raise _lib.DudfError(f"{what}: a {shape} without {plural} has no index (DUDF_E_BADCFG)")
    nbytes = _bytes(f"{prefix}_index_bytes", n, err=-4)
    index = torch.zeros(nbytes, dtype=torch.uint8, device=dev)     # zeros: the padding between the sections is part of "same bytes"
    assert index.data_ptr() % 256 == 0
    with torch.cuda.device(dev):
        if order is None:
            codes = torch.empty(n, dtype=torch.int64, device=dev)
            _call(f"{prefix}_morton_codes", _ptr(rows), n, _ptr(index), nbytes, _ptr(codes))
            order = torch.sort(codes, stable=True).indices
        elif not torch.is_tensor(order) or order.device != dev or order.dtype != torch.int64 or order.shape != (n,):
            raise _lib.DudfError(f"{what}: order must be an int64 ({letter},) CUDA tensor on the device of {arg}")
        order = order.contiguous()
        _call(f"{prefix}_index_build", _ptr(rows), n, _ptr(order), _ptr(index), nbytes)
    flags = int(index[MESH_INDEX_FLAGS_OFFSET:MESH_INDEX_FLAGS_OFFSET + 4].view(torch.int32).item())
    if flags & MESH_FLAG_NONFINITE:
        raise ValueError(f"{what}: the {shape} has a NaN or infinite {row}")
    if flags & MESH_FLAG_BAD_ORDER:
        raise _lib.DudfError(f"{what}: the sorted order is not a permutation of the {plural}")
    return index


def mesh_index_build(tri, order=None):
    """Index of a triangle soup tri (T,9) float32 for `mesh_distance`: a uint8 CUDA tensor.  Morton codes on the device, a stable
    `torch.sort`, then the boxes level by level; one host read at the end (the flag word).  ValueError for a NaN / infinite vertex.
    order (T,) int64: a permutation of the triangles to build the leaves from instead of the Morton order (any permutation gives
    the same answers, more slowly)."""
    return _index_build("mesh_index_build", "dudf_mesh", tri, 9, order, ("mesh", "vertex", "triangles", "T", "tri"))


def cloud_index_build(pc_pos, order=None):
    """Index of a point cloud pc_pos (P,3) float32 for the indexed batch sampler (`dudf_sample_batch_indexed`): a uint8 CUDA tensor.
    The mesh index's construction over points: Morton codes on the device, a stable `torch.sort`, the leaves of 8 points, then the
    boxes level by level; one host read at the end (the flag word).  ValueError for a NaN / infinite coordinate.  order (P,)
    int64: a permutation of the points to build the leaves from instead of the Morton order."""
    return _index_build("cloud_index_build", "dudf_cloud", pc_pos, 3, order, ("cloud", "coordinate", "points", "P", "pc_pos"))


def _mesh_args(what, tri, index):
    """(tri (T,9) float32, index bytes) of a mesh query: the checks `mesh_distance` makes."""
    tri = _tensor(tri, f"{what}: tri", torch.float32, (9,), convert=True)
    nbytes = 0
    if index is not None:
        if not torch.is_tensor(index) or index.device != tri.device or index.dtype != torch.uint8 or not index.is_contiguous():
            raise _lib.DudfError(f"{what}: index must be the uint8 CUDA tensor of mesh_index_build on the device of tri")
        nbytes = index.numel()
    return tri, nbytes


def mesh_occupancy(tri, index, points):
    """(count (Q,) int32, inside (Q,) uint8) for points (Q,3): how many triangles of the soup tri (T,9) the ray from each point
    along +x crosses, and its parity — `scene.compute_occupancy(points)` for a closed mesh (`dudf_mesh_occupancy`, whose comment in
    include/dudf_hip.h states the rule on edges and vertices).  index: what `mesh_index_build(tri)` returned, or None for the scan of
    every triangle (the same counts).  A NaN point: count -1, inside 0."""
    tri, nbytes = _mesh_args("mesh_occupancy", tri, index)
    points = _tensor(points, "mesh_occupancy: points", torch.float32, (3,), convert=True)
    if points.device != tri.device:
        raise _lib.DudfError("mesh_occupancy: tri and points live on different devices")
    T, Q, dev = tri.shape[0], points.shape[0], tri.device
    count = torch.empty(Q, dtype=torch.int32, device=dev)
    inside = torch.empty(Q, dtype=torch.uint8, device=dev)
    if Q and T == 0:
        _lib.check(-1, "dudf_mesh_occupancy (no triangles)")
    _call("dudf_mesh_occupancy", _ptr(tri), T, _ptr(index), nbytes, _ptr(points), Q, _ptr(count), _ptr(inside), dev=dev)
    return count, inside


def mesh_trace_rays(tri, index, rays, t0, mask, surface_eps=0.001, max_iterations=30, bound=1.3):
    """The marching loop of reference src/render_st.py:255-268 against the soup tri (T,9) in one launch (`dudf_mesh_trace_rays`):
    rays (m,3), t0 (m,3) float64 CUDA tensors, mask (m,) uint8; t0 and mask are updated in place.  Returns hits (m,) uint8.
    index: what `mesh_index_build(tri)` returned, or None for the scan of every triangle (the same bits)."""
    tri, nbytes = _mesh_args("mesh_trace_rays", tri, index)
    for name, t, dt, shape in (("rays", rays, torch.float64, (3,)), ("t0", t0, torch.float64, (3,)), ("mask", mask, torch.uint8, ())):
        if _tensor(t, f"mesh_trace_rays: {name}", dt, shape).device != tri.device:
            raise _lib.DudfError(f"mesh_trace_rays: tri and {name} live on different devices")
    m, dev = t0.shape[0], tri.device
    if rays.shape[0] != m or mask.shape[0] != m:
        raise _lib.DudfError("mesh_trace_rays: row counts of rays, t0 and mask differ")
    if int(max_iterations) < 0:
        raise _lib.DudfError(f"mesh_trace_rays: max_iterations must not be negative; got {max_iterations}")
    hits = torch.empty(m, dtype=torch.uint8, device=dev)
    if m and tri.shape[0] == 0:
        _lib.check(-1, "dudf_mesh_trace_rays (no triangles)")
    _call("dudf_mesh_trace_rays", _ptr(tri), tri.shape[0], _ptr(index), nbytes, _ptr(rays), _ptr(t0), _ptr(mask), _ptr(hits), m,
          float(surface_eps), int(max_iterations), float(bound), dev=dev)
    return hits


def mesh_distance(tri, index, points, want_idx=False, want_closest=False, stats=None):
    """(dist (Q,) float32, idx (Q,) int64 | None, closest (Q,3) float32 | None) for points (Q,3): the exact unsigned distance to
    the soup tri (T,9), the nearest triangle (smallest index among ties) and the closest point on it.  index: what
    `mesh_index_build(tri)` returned, or None for the brute-force scan (same bits).  stats: int64 CUDA tensor of 1, the number of
    exact triangle evaluations is ADDED to it."""
    tri, nbytes = _mesh_args("mesh_distance", tri, index)
    points = _tensor(points, "mesh_distance: points", torch.float32, (3,), convert=True)
    if points.device != tri.device:
        raise _lib.DudfError("mesh_distance: tri and points live on different devices")
    T, Q, dev = tri.shape[0], points.shape[0], tri.device
    if stats is not None and (not torch.is_tensor(stats) or stats.device != dev or stats.dtype != torch.int64 or stats.numel() != 1):
        raise _lib.DudfError("mesh_distance: stats must be an int64 CUDA tensor of 1")
    dist = torch.empty(Q, dtype=torch.float32, device=dev)
    idx = torch.empty(Q, dtype=torch.int64, device=dev) if want_idx else None
    closest = torch.empty(Q, 3, dtype=torch.float32, device=dev) if want_closest else None
    if Q and T == 0:
        _lib.check(-1, "dudf_mesh_distance (no triangles)")
    _call("dudf_mesh_distance", _ptr(tri), T, _ptr(index), nbytes, _ptr(points), Q, _ptr(dist), _ptr(idx), _ptr(closest),
          _ptr(stats), dev=dev)
    return dist, idx, closest
