# coding: utf-8
"""CPU: error codes of the C ABI and which of two simultaneous errors a call reports.

Every call here returns before its first HIP call, so no GPU is needed: the "device" pointers are a host address that is never
dereferenced, the workspace a 256-byte-aligned host buffer.  The expected values were recorded from the library as it stood
before the host glue was reorganised (entry points moved beside their kernels, shared checks written once); they pin the
precedence of the checks, which nothing else does."""
import ctypes
import os

import numpy as np
import pytest

from diffudf_amd import _lib
from diffudf_amd import marching_cubes as M

OK, E_CFG, E_WS, E_MODE, E_UNSUP = 0, -1, -2, -3, -4
N = 8                                                   # points / rays / rows of every call

_arena = ctypes.create_string_buffer(1 << 22)
BASE = (ctypes.addressof(_arena) + 255) // 256 * 256    # 256-byte aligned; 4 MiB - 256 bytes behind it
P = ctypes.c_void_p(BASE)                               # stands in for any device pointer (never read)
W4 = (ctypes.c_double * 4)(1.0, 1.0, 0.0, 1.0)
W4H = (ctypes.c_double * 4)(1.0, 1.0, 1.0, 1.0)         # with a Hessian weight

# the Lewiner tables' descriptors (read on the host by dudf_mc_lewiner_*; the table bytes themselves are a "device" pointer)
_z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g10_meshudf.npz"))
_, _LUT_OFFS, _LUT_DIMS = M._pack_luts({k[4:]: _z[k] for k in _z.files if k.startswith("lut_")})
LUTS = (P, ctypes.c_void_p(_LUT_OFFS.ctypes.data), ctypes.c_void_p(_LUT_DIMS.ctypes.data), len(_LUT_OFFS))


def good_cfg():
    return _lib.NetCfg(3, 2, 32, 30.0)


def ref(cfg):
    return ctypes.byref(cfg) if cfg is not None else None


# name -> (call(lib, cfg, n, ws, nbytes), need(lib, cfg, n), takes a cfg, n == 0 returns 0 before HIP)
CALLS = {
    "dudf_query": (lambda L, c, n, ws, nb: L.dudf_query(ref(c), P, P, n, P, P, ws, nb, None),
                   lambda L, c, n: L.dudf_workspace_bytes_query(ref(c), n, 0), True, True),
    "dudf_query_hessian": (lambda L, c, n, ws, nb: L.dudf_query_hessian(ref(c), P, P, n, P, P, P, ws, nb, None),
                           lambda L, c, n: L.dudf_workspace_bytes_query(ref(c), n, n), True, True),
    "dudf_query_frame": (lambda L, c, n, ws, nb: L.dudf_query_frame(ref(c), P, P, n, P, P, P, P, P, ws, nb, None),
                         lambda L, c, n: L.dudf_workspace_bytes_query(ref(c), n, n), True, True),
    "dudf_query_curvature": (lambda L, c, n, ws, nb: L.dudf_query_curvature(ref(c), P, P, n, P, P, P, P, P, ws, nb, None),
                             lambda L, c, n: L.dudf_workspace_bytes_curvature(ref(c), n), True, True),
    "dudf_trace_rays": (lambda L, c, n, ws, nb: L.dudf_trace_rays(ref(c), P, P, P, P, P, n, 0, 1.0, 0.01, 0.01, 4, 1, None, ws, nb, None),
                        lambda L, c, n: L.dudf_workspace_bytes_query(ref(c), n, 0), True, True),
    "dudf_descend_rays": (lambda L, c, n, ws, nb: L.dudf_descend_rays(ref(c), P, P, P, n, 0, 1.0, 0.01, 2, ws, nb, None),
                          lambda L, c, n: L.dudf_workspace_bytes_query(ref(c), n, 0), True, True),
    "dudf_project_points": (lambda L, c, n, ws, nb: L.dudf_project_points(ref(c), P, P, n, 1, 0, 1.0, 0.01, P, P, P, P, ws, nb, None),
                            lambda L, c, n: L.dudf_workspace_bytes_query(ref(c), n, 0), True, True),
    "dudf_pointcloud_append": (lambda L, c, n, ws, nb: L.dudf_pointcloud_append(P, n, P, P, P, P, P, P, 16, 1 << 62, P, ws, nb, None),
                               lambda L, c, n: L.dudf_pointcloud_append_workspace_bytes(n), False, True),
    "dudf_pointcloud_read_proposals": (lambda L, c, n, ws, nb: L.dudf_pointcloud_read_proposals(ref(c), n, P, ws, nb, None),
                                       lambda L, c, n: L.dudf_pointcloud_workspace_bytes(ref(c), n), True, True),
    "dudf_pointcloud_round": (lambda L, c, n, ws, nb: L.dudf_pointcloud_round(ref(c), P, n, 1, 0, 1.0, 0.01, None, 0, 0, 0, P, P, 2 * n, P, None,
                                                                            ws, nb, None),
                              lambda L, c, n: L.dudf_pointcloud_workspace_bytes(ref(c), n), True, True),
    "dudf_render_gather": (lambda L, c, n, ws, nb: L.dudf_render_gather(P, n, P, P, P, P, P, P, ws, nb, None),
                           lambda L, c, n: L.dudf_pointcloud_append_workspace_bytes(n), False, False),   # n == 0: clears its counter first
    "dudf_grid_fields": (lambda L, c, n, ws, nb: L.dudf_grid_fields(ref(c), P, 4, 0, n, 0, 1.0, P, P, P, ws, nb, None),
                         lambda L, c, n: L.dudf_workspace_bytes_query(ref(c), n, 0), True, True),
    "dudf_loss_forward": (lambda L, c, n, ws, nb: L.dudf_loss_forward(ref(c), 0, P, P, P, P, n, n, 0, W4, 1.0, P, ws, nb, None),
                          lambda L, c, n: L.dudf_workspace_bytes_hess(ref(c), n, 0), True, False),
    "dudf_s2_forward_stats": (lambda L, c, n, ws, nb: L.dudf_s2_forward_stats(ref(c), P, P, P, n, P, ws, nb, None),
                              lambda L, c, n: L.dudf_workspace_bytes(ref(c), n), True, False),
    "dudf_loss_backward": (lambda L, c, n, ws, nb: L.dudf_loss_backward(ref(c), 0, P, P, P, P, n, n, 0, W4, 1.0, P, None, P, 0, ws, nb, None),
                           lambda L, c, n: L.dudf_workspace_bytes_hess(ref(c), n, 0), True, False),
    "dudf_loss_backward_sweeps": (lambda L, c, n, ws, nb: L.dudf_loss_backward_sweeps(ref(c), 0, P, P, P, n, n, 0, W4, 1.0, P, None, ws, nb, None),
                                  lambda L, c, n: L.dudf_workspace_bytes_hess(ref(c), n, 0), True, False),
    "dudf_weight_gradient": (lambda L, c, n, ws, nb: L.dudf_weight_gradient(ref(c), n, 0, 1, 0, 1, P, 0, ws, nb, None),
                             lambda L, c, n: L.dudf_workspace_bytes_hess(ref(c), n, 0), True, False),
    "dudf_fields_forward": (lambda L, c, n, ws, nb: L.dudf_fields_forward(ref(c), P, P, n, P, P, ws, nb, None),
                            lambda L, c, n: L.dudf_workspace_bytes(ref(c), n), True, False),
    "dudf_fields_backward": (lambda L, c, n, ws, nb: L.dudf_fields_backward(ref(c), P, P, n, P, P, P, 0, ws, nb, None),
                             lambda L, c, n: L.dudf_workspace_bytes(ref(c), n), True, False),
    "dudf_debug_read_stash": (lambda L, c, n, ws, nb: L.dudf_debug_read_stash(ref(c), 0, 0, 0, n, 0, P, ws, nb, None),
                              lambda L, c, n: L.dudf_workspace_bytes_hess(ref(c), n, 0), True, False),
    "dudf_debug_loss_stage": (lambda L, c, n, ws, nb: L.dudf_debug_loss_stage(ref(c), 0, n, 0, P, P, None, P, P, n, W4, 1.0, P, None, P, None, P, P,
                                                                              None, P, ws, nb, None),
                              lambda L, c, n: L.dudf_workspace_bytes_hess(ref(c), n, 0), True, True),
    "dudf_nearest_points": (lambda L, c, n, ws, nb: L.dudf_nearest_points(P, n, P, 4, 2, P, P, ws, nb, None),
                            lambda L, c, n: L.dudf_nearest_workspace_bytes(n), False, True),
    "dudf_chamfer_terms": (lambda L, c, n, ws, nb: L.dudf_chamfer_terms(P, None, n, None, None, 0, P, ws, nb, None),
                           lambda L, c, n: L.dudf_chamfer_terms_workspace_bytes(n), False, False),
    "dudf_vertex_normals": (lambda L, c, n, ws, nb: L.dudf_vertex_normals(P, n, P, 1, P, ws, nb, None),
                            lambda L, c, n: L.dudf_vertex_normals_workspace_bytes(n), False, True),
    "dudf_mesh_morton_codes": (lambda L, c, n, ws, nb: L.dudf_mesh_morton_codes(P, n, ws, nb, P, None),
                               lambda L, c, n: L.dudf_mesh_index_bytes(n), False, False),
    "dudf_mesh_index_build": (lambda L, c, n, ws, nb: L.dudf_mesh_index_build(P, n, P, ws, nb, None),
                              lambda L, c, n: L.dudf_mesh_index_bytes(n), False, False),
    "dudf_capudf_count": (lambda L, c, n, ws, nb: L.dudf_capudf_count(P, P, n, 0.008, P, ws, nb, None),
                          lambda L, c, n: L.dudf_capudf_workspace_bytes(n), False, False),
    "dudf_capudf_emit": (lambda L, c, n, ws, nb: L.dudf_capudf_emit(P, P, n, 0.008, P, P, None, ws, nb, None),
                         lambda L, c, n: L.dudf_capudf_workspace_bytes(n), False, False),
    # the stages that arrived later: recorded from the library as it stood before they shared one workspace carver
    "dudf_mc_lewiner_count": (lambda L, c, n, ws, nb: L.dudf_mc_lewiner_count(P, n, n, n, 0.0, *LUTS, P, ws, nb, None),
                              lambda L, c, n: L.dudf_mc_lewiner_workspace_bytes(n, n, n), False, False),
    "dudf_mc_lewiner_emit": (lambda L, c, n, ws, nb: L.dudf_mc_lewiner_emit(P, n, n, n, 0.0, *LUTS, P, P, P, P, ws, nb, None),
                             lambda L, c, n: L.dudf_mc_lewiner_workspace_bytes(n, n, n), False, False),
    "dudf_mesh_clean_count": (lambda L, c, n, ws, nb: L.dudf_mesh_clean_count(P, n, P, n, 8, 0, P, ws, nb, None),
                              lambda L, c, n: L.dudf_mesh_clean_workspace_bytes(n, n), False, False),
    "dudf_mesh_clean_emit": (lambda L, c, n, ws, nb: L.dudf_mesh_clean_emit(P, n, P, n, 8, 0, P, P, ws, nb, None),
                             lambda L, c, n: L.dudf_mesh_clean_workspace_bytes(n, n), False, True),
    "dudf_mesh_border_count": (lambda L, c, n, ws, nb: L.dudf_mesh_border_count(n, P, n, P, ws, nb, None),
                               lambda L, c, n: L.dudf_mesh_border_workspace_bytes(n, n), False, False),
    "dudf_mesh_border_edges": (lambda L, c, n, ws, nb: L.dudf_mesh_border_edges(n, P, n, P, ws, nb, None),
                               lambda L, c, n: L.dudf_mesh_border_workspace_bytes(n, n), False, True),
    "dudf_mesh_smooth_borders": (lambda L, c, n, ws, nb: L.dudf_mesh_smooth_borders(P, n, P, n, 5, 0.3, ws, nb, None),
                                 lambda L, c, n: L.dudf_mesh_border_workspace_bytes(n, n), False, True),
    "dudf_knn_points[grid]": (lambda L, c, n, ws, nb: L.dudf_knn_points(P, n, P, 4, 1, 0, 0, P, P, ws, nb, None),
                              lambda L, c, n: L.dudf_knn_workspace_bytes(n, 4, 1, 0), False, True),
    "dudf_knn_points[brute]": (lambda L, c, n, ws, nb: L.dudf_knn_points(P, n, P, 4, 1, 0, 1, P, P, ws, nb, None),
                               lambda L, c, n: L.dudf_knn_workspace_bytes(n, 4, 1, 1), False, True),
    "dudf_knn_grid_build": (lambda L, c, n, ws, nb: L.dudf_knn_grid_build(P, n, ws, nb, None),
                            lambda L, c, n: L.dudf_knn_workspace_bytes(0, n, 1, 0), False, False),
    "dudf_orient_normals": (lambda L, c, n, ws, nb: L.dudf_orient_normals(P, P, P, n, 10, P, P, P, P, None, ws, nb, None),
                            lambda L, c, n: L.dudf_orient_workspace_bytes(n, 10), False, True),
}
WITH_CFG = sorted(k for k, v in CALLS.items() if v[2])
ZERO_OK = sorted(k for k, v in CALLS.items() if v[3])


def need_of(lib, name, cfg, n):
    nb = int(CALLS[name][1](lib, cfg, n))
    assert 0 < nb <= (1 << 22) - 512, (name, nb)
    return nb


@pytest.mark.parametrize("name", sorted(CALLS))
def test_workspace_null_misaligned_short(name):
    lib, cfg = _lib.load(), good_cfg()
    call = CALLS[name][0]
    nb = need_of(lib, name, cfg, N)
    assert call(lib, cfg, N, None, nb) == E_WS
    assert call(lib, cfg, N, ctypes.c_void_p(BASE + 8), nb) == E_WS
    assert call(lib, cfg, N, P, nb - 1) == E_WS


# a check BEHIND the workspace check that a call can trip without a GPU (a null output): with exactly `need` bytes the call gets
# that far, so `need` is enough for the entry point's own layout, not merely one more than what it refuses
BEHIND = {
    "dudf_capudf_count": lambda L, ws, nb: L.dudf_capudf_count(P, P, N, 0.008, None, ws, nb, None),
    "dudf_capudf_emit": lambda L, ws, nb: L.dudf_capudf_emit(P, P, N, 0.008, None, P, None, ws, nb, None),
    "dudf_mc_lewiner_count": lambda L, ws, nb: L.dudf_mc_lewiner_count(P, N, N, N, 0.0, *LUTS, None, ws, nb, None),
    "dudf_mc_lewiner_emit": lambda L, ws, nb: L.dudf_mc_lewiner_emit(P, N, N, N, 0.0, *LUTS, P, P, P, None, ws, nb, None),
    "dudf_mesh_clean_count": lambda L, ws, nb: L.dudf_mesh_clean_count(P, N, P, N, 8, 0, None, ws, nb, None),
    "dudf_mesh_clean_emit": lambda L, ws, nb: L.dudf_mesh_clean_emit(P, N, P, N, 8, 0, P, None, ws, nb, None),
    "dudf_mesh_border_count": lambda L, ws, nb: L.dudf_mesh_border_count(N, P, N, None, ws, nb, None),
    "dudf_mesh_border_edges": lambda L, ws, nb: L.dudf_mesh_border_edges(N, P, N, None, ws, nb, None),
    "dudf_mesh_smooth_borders": lambda L, ws, nb: L.dudf_mesh_smooth_borders(None, N, P, N, 5, 0.3, ws, nb, None),
}


@pytest.mark.parametrize("name", sorted(BEHIND))
def test_exactly_the_published_bytes_pass_the_workspace_check(name):
    lib = _lib.load()
    nb = need_of(lib, name, None, N)
    assert BEHIND[name](lib, P, nb) == E_CFG
    assert BEHIND[name](lib, P, nb - 1) == E_WS                 # ... and the workspace is looked at first
    assert BEHIND[name](lib, None, nb) == E_WS


@pytest.mark.parametrize("name", ["dudf_capudf_count", "dudf_capudf_emit", "dudf_mc_lewiner_count", "dudf_mc_lewiner_emit"])
def test_extraction_workspaces_are_256_byte_aligned_like_every_other(name):
    """These two stages once took any 16-byte-aligned base; include/dudf_hip.h has always asked for 256."""
    lib = _lib.load()
    nb = need_of(lib, name, None, N)
    assert CALLS[name][0](lib, None, N, ctypes.c_void_p(BASE + 16), nb) == E_WS
    assert CALLS[name][0](lib, None, N, ctypes.c_void_p(BASE + 128), nb) == E_WS


def test_mesh_distance_index_is_optional_but_checked():
    lib = _lib.load()
    nb = int(lib.dudf_mesh_index_bytes(N))
    dist = lambda index, nbytes, q=N: lib.dudf_mesh_distance(P, N, index, nbytes, P, q, P, None, None, None, None)  # noqa: E731
    assert dist(ctypes.c_void_p(BASE + 8), nb) == E_WS
    assert dist(P, nb - 1) == E_WS
    assert dist(None, 0, 0) == OK
    assert dist(P, nb, -1) == E_CFG
    assert lib.dudf_mesh_distance(None, N, P, nb, P, N, P, None, None, None, None) == E_CFG


# a bad cfg: null, and a width no kernel is built for.  The byte-count queries answer 0, the counts -1.
BAD_CFG_EXPECT = {name: E_CFG for name in WITH_CFG}


@pytest.mark.parametrize("name", WITH_CFG)
@pytest.mark.parametrize("bad", ["null", "width100"])
def test_bad_cfg(name, bad):
    lib = _lib.load()
    nb = need_of(lib, name, good_cfg(), N)
    cfg = None if bad == "null" else _lib.NetCfg(3, 2, 100, 30.0)
    assert CALLS[name][0](lib, cfg, N, P, nb) == BAD_CFG_EXPECT[name]


@pytest.mark.parametrize("bad", ["null", "width100"])
def test_bad_cfg_of_the_host_only_calls(bad):
    lib = _lib.load()
    cfg = None if bad == "null" else _lib.NetCfg(3, 2, 100, 30.0)
    c = ref(cfg)
    assert lib.dudf_theta_count(c) == -1
    assert lib.dudf_stash_mode(c, N, 0) == -1
    assert lib.dudf_sweeps_bf16x6(c) == 0
    assert lib.dudf_workspace_bytes(c, N) == 0
    assert lib.dudf_workspace_bytes_hess(c, N, 0) == 0
    assert lib.dudf_workspace_bytes_query(c, N, 0) == 0
    assert lib.dudf_workspace_bytes_curvature(c, N) == 0
    assert lib.dudf_pointcloud_workspace_bytes(c, N) == 0
    out = (ctypes.c_int64 * 10)()
    assert lib.dudf_debug_stash_layout(c, N, 0, out) == E_CFG
    name = ctypes.create_string_buffer(128)
    assert lib.dudf_debug_kernel_choice(c, N, 0, 0, 0, name, 128) == E_CFG


@pytest.mark.parametrize("name", ZERO_OK)
def test_zero_count_returns_before_any_work(name):
    lib, cfg = _lib.load(), good_cfg()
    nb = need_of(lib, name, cfg, 0)
    assert CALLS[name][0](lib, cfg, 0, P, nb) == OK


def test_byte_counts_agree():
    lib, cfg = _lib.load(), good_cfg()
    assert lib.dudf_workspace_bytes(ref(cfg), N) == lib.dudf_workspace_bytes_hess(ref(cfg), N, 0) > 0
    assert lib.dudf_workspace_bytes_hess(ref(cfg), N, N + 1) == 0
    assert lib.dudf_workspace_bytes_query(ref(cfg), N, N + 1) == 0
    assert lib.dudf_workspace_bytes_curvature(ref(cfg), -1) == 0
    assert lib.dudf_pointcloud_append_workspace_bytes(-1) == 0
    assert lib.dudf_pointcloud_workspace_bytes(ref(cfg), -1) == 0


# ---- two errors at once: which one is reported --------------------------------------------------------------------------------
def test_trace_rays_bad_mode_wins_over_null_cfg():
    lib, cfg = _lib.load(), good_cfg()
    nb = need_of(lib, "dudf_trace_rays", cfg, N)
    trace = lambda c, mode, max_it=4, every=1, ws=P: lib.dudf_trace_rays(c, P, P, P, P, P, N, mode, 1.0, 0.01, 0.01, max_it, every,  # noqa: E731
                                                                         None, ws, nb, None)
    assert trace(None, 3) == E_MODE
    assert trace(None, -1) == E_MODE
    assert trace(ref(cfg), 0, -1) == E_MODE
    assert trace(ref(cfg), 0, 4, 0) == E_MODE
    assert trace(None, 0) == E_CFG
    assert trace(None, 0, ws=None) == E_CFG             # cfg before workspace
    assert trace(ref(cfg), 3, ws=None) == E_MODE


def test_descend_and_project_mode_before_cfg_and_workspace():
    lib, cfg = _lib.load(), good_cfg()
    nb = need_of(lib, "dudf_descend_rays", cfg, N)
    assert lib.dudf_descend_rays(None, P, P, P, N, 3, 1.0, 0.01, 2, None, nb, None) == E_MODE
    assert lib.dudf_descend_rays(ref(cfg), P, P, P, N, 0, 1.0, 0.01, -1, P, nb, None) == E_MODE
    assert lib.dudf_descend_rays(None, P, P, P, N, 0, 1.0, 0.01, 2, None, nb, None) == E_CFG
    assert lib.dudf_project_points(None, P, P, N, 1, 3, 1.0, 0.01, P, P, P, P, None, nb, None) == E_MODE
    assert lib.dudf_project_points(ref(cfg), P, P, N, 0, 0, 1.0, 0.01, P, P, P, P, P, nb, None) == E_MODE
    assert lib.dudf_project_points(None, P, P, N, 1, 0, 1.0, 0.01, P, P, P, P, None, nb, None) == E_CFG


def test_pointcloud_round_precedence():
    lib, cfg = _lib.load(), good_cfg()
    nb = need_of(lib, "dudf_pointcloud_round", cfg, N)
    rnd = lambda c, mode, steps, ws, nbytes, counter=P, capacity=2 * N, pts=P, nrm=P: lib.dudf_pointcloud_round(  # noqa: E731
        c, P, N, steps, mode, 1.0, 0.01, None, 0, 0, 0, pts, nrm, capacity, counter, None, ws, nbytes, None)
    assert rnd(ref(cfg), 3, 1, P, nb - 1) == E_MODE             # bad mode + short workspace
    assert rnd(ref(cfg), 0, 0, P, nb - 1) == E_MODE             # no steps + short workspace
    assert rnd(None, 3, 1, P, nb) == E_MODE                     # bad mode + null cfg
    assert rnd(None, 0, 1, None, nb) == E_CFG                   # null cfg + null workspace
    assert rnd(ref(cfg), 0, 1, P, nb - 1, counter=None) == E_WS  # short workspace + null counter
    assert rnd(ref(cfg), 0, 1, P, nb, counter=None) == E_CFG
    assert rnd(ref(cfg), 0, 1, P, nb, pts=None) == E_CFG
    assert rnd(ref(cfg), 0, 1, P, nb, nrm=None) == E_CFG
    assert rnd(ref(cfg), 0, 1, P, nb, capacity=2 * N - 1) == E_CFG


def test_pointcloud_append_precedence():
    lib = _lib.load()
    nb = need_of(lib, "dudf_pointcloud_append", None, N)
    app = lambda n, ws, flags=P, src=P, dst=P, counter=P, capacity=16: lib.dudf_pointcloud_append(  # noqa: E731
        flags, n, src, P, P, dst, P, P, capacity, 1 << 62, counter, ws, nb, None)
    assert app(-1, None) == E_CFG                               # negative n + null workspace
    assert app(N, None, counter=None) == E_CFG                  # null counter + null workspace
    assert app(N, P, capacity=-1) == E_CFG
    assert app((1 << 30) + 1, P) == E_CFG
    assert app(N, None, flags=None) == E_WS                     # the row pointers are looked at after the workspace
    assert app(N, P, flags=None) == E_CFG
    assert app(N, P, src=None) == E_CFG
    assert app(N, P, dst=None) == E_CFG
    assert app(0, P, flags=None) == OK                          # ... and not at all for an empty call
    assert lib.dudf_pointcloud_read_proposals(ref(good_cfg()), N, None, P, need_of(lib, "dudf_pointcloud_read_proposals", good_cfg(), N),
                                              None) == E_CFG
    assert lib.dudf_pointcloud_read_proposals(ref(good_cfg()), N, None, None, 0, None) == E_WS


def test_loss_mode_checks_and_their_precedence():
    lib, cfg = _lib.load(), good_cfg()
    nb = need_of(lib, "dudf_loss_backward", cfg, N)
    fwd = lambda c, mode, ws, n_hess=0, w=W4: lib.dudf_loss_forward(c, mode, P, P, P, P, N, N, n_hess, w, 1.0, P, ws, nb, None)  # noqa: E731
    bwd = lambda c, mode, ws, n_hess=0, w=W4, stats=None: lib.dudf_loss_backward(c, mode, P, P, P, P, N, N, n_hess, w, 1.0, P, stats, P, 0,  # noqa: E731
                                                                                 ws, nb, None)
    bws = lambda c, mode, ws, n_hess=0, w=W4, stats=None: lib.dudf_loss_backward_sweeps(c, mode, P, P, P, N, N, n_hess, w, 1.0, P, stats,  # noqa: E731
                                                                                        ws, nb, None)
    assert bwd(ref(cfg), 7, None) == E_MODE                     # bad mode + null workspace
    assert bwd(None, 7, None) == E_MODE                         # bad mode + null cfg
    assert bwd(None, 0, None) == E_CFG                          # null cfg + null workspace
    assert fwd(ref(cfg), _lib.LOSS_S2, P) == E_MODE             # the forward takes two modes ...
    assert fwd(ref(cfg), 7, None) == E_MODE
    assert fwd(None, 0, None) == E_CFG
    for back in (bwd, bws):                                     # ... the backward three; s2 needs its statistics
        assert back(ref(cfg), _lib.LOSS_S2, None) == E_MODE
        assert back(ref(cfg), _lib.LOSS_S2, None, stats=P) == E_WS
        assert back(ref(cfg), 7, None, stats=P) == E_MODE
        assert back(ref(cfg), -1, P) == E_MODE
    # Hessian-path points only with loss_s1 and a Hessian weight
    for f in (fwd, bwd, bws):
        assert f(ref(cfg), _lib.LOSS_S1, None, n_hess=2, w=W4) == E_MODE
        assert f(ref(cfg), _lib.LOSS_SIREN, None, n_hess=2, w=W4H) == E_MODE
        assert f(ref(cfg), _lib.LOSS_S1, None, n_hess=2, w=W4H) == E_WS
        assert f(None, _lib.LOSS_S1, None, n_hess=2, w=W4) == E_MODE
        assert f(ref(cfg), _lib.LOSS_S1, P, n_hess=N + 1, w=W4H) == E_CFG       # more Hessian points than points


def test_query_curvature_checks_the_whole_workspace():
    lib, cfg = _lib.load(), good_cfg()
    full = int(lib.dudf_workspace_bytes_curvature(ref(cfg), N))
    query_part = int(lib.dudf_workspace_bytes_query(ref(cfg), N, N))
    assert 0 < query_part < full
    curv = lambda c, n, ws, nbytes: lib.dudf_query_curvature(c, P, P, n, P, P, P, P, P, ws, nbytes, None)  # noqa: E731
    assert curv(ref(cfg), N, P, query_part) == E_WS             # enough for the Hessian query, not for the jets
    assert curv(ref(cfg), N, P, full - 1) == E_WS
    assert curv(None, N, None, 0) == E_CFG
    assert curv(ref(cfg), -1, None, 0) == E_CFG
    assert curv(ref(cfg), 0, None, 0) == E_WS                   # the workspace is checked before the empty call returns
    assert curv(ref(cfg), (1 << 21) + 1, P, 1 << 20) == E_CFG   # 16 jet columns per point: past 2^25 columns


# ---- range checks ------------------------------------------------------------------------------------------------------------
def test_weight_gradient_layer_ranges():
    lib, cfg = _lib.load(), good_cfg()
    nb = need_of(lib, "dudf_weight_gradient", cfg, N)
    wg = lambda b, e, ws=P: lib.dudf_weight_gradient(ref(cfg), N, 0, 1, b, e, P, 0, ws, nb, None)  # noqa: E731
    assert wg(1, 1) == E_CFG
    assert wg(2, 1) == E_CFG
    assert wg(-2, 1) == E_CFG
    assert wg(0, cfg.n_hidden_layers + 2) == E_CFG
    assert wg(1, 1, None) == E_WS                               # the workspace before the range


def test_grid_fields_ranges():
    lib, cfg = _lib.load(), good_cfg()
    nb = need_of(lib, "dudf_grid_fields", cfg, N)
    gf = lambda c, grid_n, start, count, mode, ws=P: lib.dudf_grid_fields(c, P, grid_n, start, count, mode, 1.0, P, P, P, ws, nb, None)  # noqa: E731
    assert gf(ref(cfg), 1, 0, 1, 0) == E_CFG
    assert gf(ref(cfg), 4, 60, 5, 0) == E_CFG                   # 64 grid points
    assert gf(ref(cfg), 4, -1, 5, 0) == E_CFG
    assert gf(ref(cfg), 4, 0, -1, 0) == E_CFG
    assert gf(ref(cfg), 1, 0, 1, 3) == E_CFG                    # the grid before the mode
    assert gf(ref(cfg), 4, 0, N, 3) == E_MODE
    assert gf(None, 4, 0, N, 3, None) == E_MODE                 # the mode before cfg and workspace
    assert gf(None, 4, 0, N, 0, None) == E_CFG


def test_render_checks():
    lib = _lib.load()
    D3 = (ctypes.c_double * 3)(0.0, 0.0, 1.0)
    shade = lambda model, m, k, hits=P, rows=P, pc1=P, camera=D3, light=D3, acc=P: lib.dudf_render_shade(  # noqa: E731
        model, hits, m, rows, k, P, P, pc1, P, None, light, camera, 1.0, 0.1, 0.1, acc, None)
    assert shade(0, 4, 5) == E_CFG                              # k > m
    assert shade(7, 4, 2) == E_MODE
    assert shade(7, 4, 5) == E_MODE                             # the model before the counts
    assert shade(0, -1, 0) == E_CFG
    assert shade(0, 4, 2, rows=None) == E_CFG
    assert shade(0, 4, 2, hits=None) == E_CFG
    assert shade(0, 4, 2, light=None) == E_CFG
    assert shade(1, 4, 2, camera=None) == E_CFG
    assert shade(1, 4, 2, pc1=None) == E_CFG
    assert shade(0, 0, 0, hits=None) == OK
    assert lib.dudf_render_finish(P, N, 0.0, P, None) == E_CFG
    assert lib.dudf_render_finish(P, N, float("nan"), P, None) == E_CFG
    assert lib.dudf_render_finish(P, -1, 1.0, P, None) == E_CFG
    assert lib.dudf_render_finish(None, N, 1.0, P, None) == E_CFG
    assert lib.dudf_render_finish(None, 0, 1.0, None, None) == OK
    R9 = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    PL = (ctypes.c_double * 6)(1, -1, 1, -1, 1, -1)
    assert lib.dudf_render_setup_rays(0, 4, 60.0, 0.5, R9, D3, PL, P, P, P, None) == E_CFG
    assert lib.dudf_render_setup_rays(4, 4, 60.0, 0.5, None, D3, PL, P, P, P, None) == E_CFG
    assert lib.dudf_render_setup_rays(4, 4, 60.0, 0.5, R9, D3, PL, None, P, P, None) == E_CFG
    assert lib.dudf_render_setup_rays(1 << 16, 1 << 16, 60.0, 0.5, R9, D3, PL, P, P, P, None) == E_CFG
    nb = need_of(lib, "dudf_render_gather", None, N)
    assert lib.dudf_render_gather(P, -1, P, P, P, P, P, P, None, nb, None) == E_CFG       # the count before the workspace
    assert lib.dudf_render_gather(P, N, P, P, P, P, P, None, None, nb, None) == E_CFG     # the counter before the workspace
    assert lib.dudf_render_orient(P, P, P, N, P, P, P, P, None) == E_CFG                  # exactly one of frame / gradient
    assert lib.dudf_render_orient(None, None, P, N, P, P, P, P, None) == E_CFG
    assert lib.dudf_render_orient(P, None, None, N, P, P, P, P, None) == E_CFG
    assert lib.dudf_render_orient(P, None, P, -1, P, P, P, P, None) == E_CFG
    assert lib.dudf_render_orient(P, None, P, 0, P, P, P, P, None) == OK
    assert lib.dudf_render_colormap(P, N, None, P, P, None) == E_CFG
    assert lib.dudf_render_colormap(None, N, P, P, P, None) == E_CFG
    assert lib.dudf_render_colormap(None, 0, P, P, None, None) == OK


def test_adam_checks():
    lib = _lib.load()
    assert lib.dudf_adam_step(P, P, P, P, N, 1e-4, 0.9, 0.999, 1e-8, 0, 1.0, None) == E_CFG
    assert lib.dudf_adam_step(P, P, P, P, 0, 1e-4, 0.9, 0.999, 1e-8, 1, 1.0, None) == E_CFG
    assert lib.dudf_adam_step_scheduled(P, P, P, P, N, 0.9, 0.999, 1e-8, None, 4, P, 1.0, None) == E_CFG
    assert lib.dudf_adam_step_scheduled(P, P, P, P, N, 0.9, 0.999, 1e-8, P, 4, None, 1.0, None) == E_CFG
    assert lib.dudf_adam_step_scheduled(P, P, P, P, N, 0.9, 0.999, 1e-8, P, 0, P, 1.0, None) == E_CFG
    assert lib.dudf_adam_step_scheduled(P, P, P, P, 0, 0.9, 0.999, 1e-8, P, 4, P, 1.0, None) == E_CFG
    assert lib.dudf_adam_schedule(None, 0, 1, 0.9, 0.999, P) == E_CFG
    assert lib.dudf_adam_schedule(None, 0, 1, 0.9, 0.999, None) == E_CFG


def test_debug_read_stash_ranges():
    lib, cfg = _lib.load(), good_cfg()
    nb = need_of(lib, "dudf_debug_read_stash", cfg, N)
    rs = lambda which, layer, channel=0, ws=P: lib.dudf_debug_read_stash(ref(cfg), which, layer, channel, N, 0, P, ws, nb, None)  # noqa: E731
    assert rs(8, 0) == E_MODE
    assert rs(-1, 0) == E_MODE
    assert rs(0, cfg.n_hidden_layers) == E_CFG
    assert rs(0, -1) == E_CFG
    assert rs(0, 0, 4) == E_CFG
    assert rs(8, cfg.n_hidden_layers) == E_CFG                  # the layer before the array
    assert rs(8, 0, 0, None) == E_WS                            # the workspace before both
    out = (ctypes.c_int64 * 10)()
    assert lib.dudf_debug_stash_layout(ref(cfg), N, 0, None) == E_CFG
    assert lib.dudf_debug_stash_layout(ref(cfg), N, 0, out) == OK
    assert lib.dudf_debug_kernel_choice(ref(cfg), N, 0, 0, 0, None, 0) == E_CFG


def test_debug_loss_stage_and_eigh3_refusals():
    """Every refusal comes before any device work: the pointers are host addresses no kernel could read, and there is no GPU here."""
    lib, cfg = _lib.load(), good_cfg()
    nb = need_of(lib, "dudf_debug_loss_stage", cfg, N)
    nbh = int(lib.dudf_workspace_bytes_hess(ref(cfg), N, 2))
    assert 0 < nbh <= (1 << 22) - 512

    def stage(c=cfg, mode=_lib.LOSS_S1, n=N, n_hess=0, w=W4, ws=P, nbytes=nb, n_global=N, **null):
        a = {k: (None if k in null else P) for k in ("y", "g", "h", "normals", "sdf", "cot", "stats_in", "out_terms", "out_stats", "out_ybar",
                                                    "out_gbar", "out_hbar", "out_pad")}
        return lib.dudf_debug_loss_stage(ref(c), mode, n, n_hess, a["y"], a["g"], a["h"], a["normals"], a["sdf"], n_global, w, 1.0, a["cot"],
                                         a["stats_in"], a["out_terms"], a["out_stats"], a["out_ybar"], a["out_gbar"], a["out_hbar"],
                                         a["out_pad"], ws, nbytes, None)

    # check_loss_mode's rules, in front of cfg and workspace as in dudf_loss_backward
    assert stage(mode=7, ws=None) == E_MODE
    assert stage(c=None, mode=-1, ws=None) == E_MODE
    assert stage(mode=_lib.LOSS_S2, out_stats=None, ws=None) == E_MODE             # loss_s2 needs somewhere for its statistics
    assert stage(mode=_lib.LOSS_S2, ws=None) == E_WS
    assert stage(mode=_lib.LOSS_S1, n_hess=2, w=W4, ws=None) == E_MODE             # Hessian-path points without a Hessian weight
    assert stage(mode=_lib.LOSS_SIREN, n_hess=2, w=W4H, ws=None) == E_MODE
    assert stage(mode=_lib.LOSS_S2, n_hess=2, w=W4H, ws=None) == E_MODE
    assert stage(mode=_lib.LOSS_S1, n_hess=2, w=W4H, ws=None) == E_WS
    assert stage(w=None, mode=7, ws=None) == E_CFG                                  # the weights are read by the mode check
    # cfg and the counts, then the workspace
    assert stage(c=None, ws=None) == E_CFG
    assert stage(n_hess=N + 1, w=W4H) == E_CFG                                     # more Hessian points than points
    assert stage(n=-1) == E_CFG
    assert stage(nbytes=nb - 1) == E_WS
    assert stage(ws=ctypes.c_void_p(BASE + 8)) == E_WS
    assert stage(n_hess=2, w=W4H, nbytes=nbh - 1) == E_WS
    assert stage(y=None, ws=None) == E_WS                                          # the workspace before the row pointers
    # an empty call succeeds without looking at its pointers; a call with points needs them all
    assert stage(n=0, n_global=0, y=None, g=None, sdf=None, out_terms=None, out_pad=None) == OK
    assert stage(n_global=0) == E_CFG
    for name in ("y", "g", "normals", "sdf", "cot", "out_terms", "out_ybar", "out_gbar", "out_pad"):
        assert stage(**{name: None}) == E_CFG, name
    assert stage(mode=_lib.LOSS_S2, stats_in=None, y=None) == E_CFG                # (stats_in itself is optional)
    for name in ("h", "out_hbar"):                                                 # needed with Hessian-path points only
        assert stage(n_hess=2, w=W4H, nbytes=nbh, **{name: None}) == E_CFG, name
    # the eigensolver: no workspace, three device pointers
    assert lib.dudf_debug_eigh3(P, -1, P, P, None) == E_CFG
    assert lib.dudf_debug_eigh3(None, 0, None, None, None) == OK
    for args in ((None, N, P, P), (P, N, None, P), (P, N, P, None)):
        assert lib.dudf_debug_eigh3(*args, None) == E_CFG


def test_chamfer_and_nearest_precedence():
    lib = _lib.load()
    nb = need_of(lib, "dudf_nearest_points", None, N)
    near = lambda n, m, norm, ws, x=P: lib.dudf_nearest_points(x, n, P, m, norm, P, P, ws, nb, None)  # noqa: E731
    assert near(N, 4, 3, None) == E_MODE
    assert near(-1, 4, 2, None) == E_CFG
    assert near(1 << 31, 4, 2, None) == E_UNSUP
    assert near(N, 0, 2, None) == E_CFG                         # the sets before the workspace
    assert near(N, 4, 2, None, x=None) == E_CFG
    assert lib.dudf_chamfer_terms(P, None, N, P, None, 4, P, None, 0, None) == E_CFG      # normals come together
    assert lib.dudf_chamfer_terms(P, None, N, P, P, 4, P, None, 0, None) == E_CFG         # ... and need idx
    assert lib.dudf_chamfer_terms(P, None, N, None, None, 0, None, None, 0, None) == E_CFG
    assert lib.dudf_vertex_normals(P, -1, P, 1, P, None, 0, None) == E_CFG
    assert lib.dudf_vertex_normals(None, N, P, 1, P, None, 0, None) == E_CFG
    assert lib.dudf_mesh_morton_codes(None, N, None, 0, P, None) == E_CFG
    assert lib.dudf_mesh_index_build(P, 0, P, None, 0, None) == E_CFG
    assert lib.dudf_mesh_index_build(P, 1 << 31, P, None, 0, None) == E_UNSUP


# ---- options ------------------------------------------------------------------------------------------------------------------
def test_option_errors():
    lib = _lib.load()
    v = ctypes.c_int(-7)
    try:
        assert lib.dudf_set_option(None, 1) == E_MODE
        assert lib.dudf_get_option(None, ctypes.byref(v)) == E_MODE
        assert lib.dudf_get_option(b"stash", None) == E_MODE
        assert lib.dudf_set_option(b"nonsense", 1) == E_MODE
        assert lib.dudf_get_option(b"nonsense", ctypes.byref(v)) == E_MODE and v.value == -7
        assert lib.dudf_set_option(b"deterministic", 2) == E_CFG
        assert lib.dudf_set_option(b"deterministic", -1) == E_CFG
        assert lib.dudf_set_option(b"wgrad_family", 3) == E_CFG
        assert lib.dudf_set_option(b"wgrad_max_workgroups", 7) == E_CFG
        assert lib.dudf_set_option(b"wgrad_max_workgroups", 257) == E_CFG
        assert lib.dudf_set_option(b"wgrad_buffers", 2) == E_CFG
        assert lib.dudf_set_option(b"stash", 16) == E_CFG
        for bad in (1, 2, 3, 4, 5, 8, 15):
            assert lib.dudf_set_option(b"stash", bad) == E_CFG
        for good in (0, 6, 7):
            assert lib.dudf_set_option(b"stash", good) == OK
            assert lib.dudf_get_option(b"stash", ctypes.byref(v)) == OK and v.value == good
        assert lib.dudf_set_wgrad_max_workgroups(7) == E_CFG
    finally:
        assert lib.dudf_reset_options() == OK
    defaults = {"deterministic": 0, "split": 1, "split_quads": 1, "sweep_family": 1, "stash": 7, "wgrad_family": 0, "wgrad_tr": 0,
                "pair_launch": 1, "wgrad_max_workgroups": 256, "wgrad_buffers": 4}
    for name, want in defaults.items():
        assert lib.dudf_get_option(name.encode(), ctypes.byref(v)) == OK and v.value == want, name
