# coding: utf-8
"""ctypes binding of libdudf_hip.so (C ABI declared in include/dudf_hip.h).

There is no CPU fallback: if the library is missing or a call fails, this module raises.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# DUDF_LIB: another build of the same library (the DUDF_FX_CHECK build of tools/build_dbg.sh; a parent build for A/B runs); default: the in-tree one
LIB_PATH = os.environ.get("DUDF_LIB") or os.path.join(_HERE, "libdudf_hip.so")

LOSS_S1, LOSS_S2, LOSS_SIREN = 0, 1, 2

_ERRORS = {
    -1: "DUDF_E_BADCFG: unsupported network (kernel width in {32,64,128,256,512} — hip_ops pads narrower / unequal layers —, n_in=3, n_out=1)",
    -2: "DUDF_E_WORKSPACE: workspace too small or misaligned",
    -3: "DUDF_E_BADMODE",
    -4: "DUDF_E_UNSUPPORTED: this configuration has no HIP path; there is deliberately no CPU fallback",
}


class NetCfg(ctypes.Structure):
    _fields_ = [("n_in", ctypes.c_int32), ("n_hidden_layers", ctypes.c_int32),
                ("hidden", ctypes.c_int32), ("w0", ctypes.c_float), ("ww", ctypes.c_float)]     # ww = 0: the same as w0


class DudfError(RuntimeError):
    pass


_lib = None

# every symbol include/dudf_hip.h declares: (restype, argtypes)
_P = ctypes.c_void_p
_CFG = ctypes.POINTER(NetCfg)
_DBL = ctypes.POINTER(ctypes.c_double)
SYMBOLS = {
    "dudf_version": (ctypes.c_char_p, []),
    "dudf_sweeps_bf16x6": (ctypes.c_int, [_CFG]),
    "dudf_theta_count": (ctypes.c_int64, [_CFG]),
    "dudf_workspace_bytes": (ctypes.c_size_t, [_CFG, ctypes.c_int64]),
    "dudf_workspace_bytes_hess": (ctypes.c_size_t, [_CFG, ctypes.c_int64, ctypes.c_int64]),
    "dudf_workspace_bytes_query": (ctypes.c_size_t, [_CFG, ctypes.c_int64, ctypes.c_int64]),
    "dudf_query_frame": (ctypes.c_int, [_CFG, _P, _P, ctypes.c_int64, _P, _P, _P, _P, _P, _P, ctypes.c_size_t, _P]),
    "dudf_workspace_bytes_curvature": (ctypes.c_size_t, [_CFG, ctypes.c_int64]),
    "dudf_query_curvature": (ctypes.c_int, [_CFG, _P, _P, ctypes.c_int64, _P, _P, _P, _P, _P, _P, ctypes.c_size_t, _P]),
    "dudf_trace_rays": (ctypes.c_int, [_CFG, _P, _P, _P, _P, _P, ctypes.c_int64, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                       ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int), _P,
                                       ctypes.c_size_t, _P]),
    "dudf_descend_rays": (ctypes.c_int, [_CFG, _P, _P, _P, ctypes.c_int64, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                         ctypes.c_int, _P, ctypes.c_size_t, _P]),
    "dudf_project_points": (ctypes.c_int, [_CFG, _P, _P, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                           _P, _P, _P, _P, _P, ctypes.c_size_t, _P]),
    "dudf_pointcloud_append_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64]),
    "dudf_pointcloud_append": (ctypes.c_int, [_P, ctypes.c_int64, _P, _P, _P, _P, _P, _P, ctypes.c_int64, ctypes.c_int64, _P, _P,
                                              ctypes.c_size_t, _P]),
    "dudf_pointcloud_workspace_bytes": (ctypes.c_size_t, [_CFG, ctypes.c_int64]),
    "dudf_pointcloud_read_proposals": (ctypes.c_int, [_CFG, ctypes.c_int64, _P, _P, ctypes.c_size_t, _P]),
    "dudf_pointcloud_round": (ctypes.c_int, [_CFG, _P, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                             _P, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int64, _P, _P, ctypes.c_int64, _P,
                                             ctypes.POINTER(ctypes.c_int64), _P, ctypes.c_size_t, _P]),
    "dudf_render_setup_rays": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64, ctypes.c_double, ctypes.c_double, _DBL, _DBL, _DBL,
                                              _P, _P, _P, _P]),
    "dudf_render_gather": (ctypes.c_int, [_P, ctypes.c_int64, _P, _P, _P, _P, _P, _P, _P, ctypes.c_size_t, _P]),
    "dudf_render_orient": (ctypes.c_int, [_P, _P, _P, ctypes.c_int64, _P, _P, _P, _P, _P]),
    "dudf_render_colormap": (ctypes.c_int, [_P, ctypes.c_int64, _P, _P, _P, _P]),
    "dudf_render_shade": (ctypes.c_int, [ctypes.c_int, _P, ctypes.c_int64, _P, ctypes.c_int64, _P, _P, _P, _P, _P, _DBL, _DBL,
                                         ctypes.c_double, ctypes.c_double, ctypes.c_double, _P, _P]),
    "dudf_render_finish": (ctypes.c_int, [_P, ctypes.c_int64, ctypes.c_double, _P, _P]),
    "dudf_nearest_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64]),
    "dudf_nearest_points": (ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_int64, ctypes.c_int, _P, _P, _P, ctypes.c_size_t, _P]),
    "dudf_chamfer_terms_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64]),
    "dudf_chamfer_terms": (ctypes.c_int, [_P, _P, ctypes.c_int64, _P, _P, ctypes.c_int64, _P, _P, ctypes.c_size_t, _P]),
    "dudf_vertex_normals_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64]),
    "dudf_vertex_normals": (ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_int64, _P, _P, ctypes.c_size_t, _P]),
    "dudf_mesh_sample_surface_workspace": (ctypes.c_size_t, [ctypes.c_int64]),
    "dudf_mesh_sample_surface": (ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_uint64,
                                                _P, _P, _P, _P, _P, _P, _P, ctypes.c_size_t, _P]),
    "dudf_distance_stats_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64]),
    "dudf_distance_stats": (ctypes.c_int, [_P, ctypes.c_int64, _DBL, ctypes.c_int, _P, _P, _P, _P, ctypes.c_size_t, _P]),
    "dudf_knn_workspace_bytes":(ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int]),
    "dudf_knn_grid_build": (ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_size_t, _P]),
    "dudf_knn_points": (ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P, _P,
                                       ctypes.c_size_t, _P]),
    "dudf_orient_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int]),
    "dudf_orient_normals": (ctypes.c_int, [_P, _P, _P, ctypes.c_int64, ctypes.c_int, _P, _P, _P, _P, ctypes.POINTER(ctypes.c_int64), _P,
                                           ctypes.c_size_t, _P]),
    "dudf_estimate_normals_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int]),
    "dudf_estimate_normals": (ctypes.c_int, [_P, _P, ctypes.c_int64, ctypes.c_int, ctypes.c_int, _P, _P, _P, _P, ctypes.c_size_t, _P]),
    "dudf_cloud_outliers_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int]),
    "dudf_cloud_outliers": (ctypes.c_int, [_P, ctypes.c_int64, ctypes.c_int, ctypes.c_double, _P, _P, _P, _P, _P, _P, ctypes.c_size_t, _P]),
    "dudf_mesh_index_bytes": (ctypes.c_size_t, [ctypes.c_int64]),
    "dudf_mesh_morton_codes": (ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_size_t, _P, _P]),
    "dudf_mesh_index_build": (ctypes.c_int, [_P, ctypes.c_int64, _P, _P, ctypes.c_size_t, _P]),
    "dudf_mesh_distance": (ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_size_t, _P, ctypes.c_int64, _P, _P, _P, _P, _P]),
    "dudf_mesh_occupancy": (ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_size_t, _P, ctypes.c_int64, _P, _P, _P]),
    "dudf_mesh_trace_rays": (ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_size_t, _P, _P, _P, _P, ctypes.c_int64, ctypes.c_double,
                                            ctypes.c_int, ctypes.c_double, _P]),
    "dudf_grid_fields": (ctypes.c_int, [_CFG, _P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
                                        ctypes.c_double, _P, _P, _P, _P, ctypes.c_size_t, _P]),
    "dudf_query": (ctypes.c_int, [_CFG, _P, _P, ctypes.c_int64, _P, _P, _P, ctypes.c_size_t, _P]),
    "dudf_query_hessian": (ctypes.c_int, [_CFG, _P, _P, ctypes.c_int64, _P, _P, _P, _P, ctypes.c_size_t, _P]),
    "dudf_loss_forward": (ctypes.c_int, [_CFG, ctypes.c_int, _P, _P, _P, _P, ctypes.c_int64, ctypes.c_int64,
                                         ctypes.c_int64, _DBL, ctypes.c_double, _P, _P, ctypes.c_size_t, _P]),
    "dudf_s2_forward_stats": (ctypes.c_int, [_CFG, _P, _P, _P, ctypes.c_int64, _P, _P, ctypes.c_size_t, _P]),
    "dudf_s2_terms": (ctypes.c_int, [_P, _DBL, _P, _P]),
    "dudf_loss_backward": (ctypes.c_int, [_CFG, ctypes.c_int, _P, _P, _P, _P, ctypes.c_int64, ctypes.c_int64,
                                          ctypes.c_int64, _DBL, ctypes.c_double, _P, _P, _P, ctypes.c_int, _P,
                                          ctypes.c_size_t, _P]),
    "dudf_loss_backward_sweeps": (ctypes.c_int, [_CFG, ctypes.c_int, _P, _P, _P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                                 _DBL, ctypes.c_double, _P, _P, _P, ctypes.c_size_t, _P]),
    "dudf_weight_gradient": (ctypes.c_int, [_CFG, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P,
                                            ctypes.c_int, _P, ctypes.c_size_t, _P]),
    "dudf_fields_forward": (ctypes.c_int, [_CFG, _P, _P, ctypes.c_int64, _P, _P, _P, ctypes.c_size_t, _P]),
    "dudf_fields_backward": (ctypes.c_int, [_CFG, _P, _P, ctypes.c_int64, _P, _P, _P, ctypes.c_int, _P,
                                            ctypes.c_size_t, _P]),
    "dudf_adam_step": (ctypes.c_int, [_P, _P, _P, _P, ctypes.c_int64, ctypes.c_double, ctypes.c_double,
                                      ctypes.c_double, ctypes.c_double, ctypes.c_int64, ctypes.c_double, _P]),
    "dudf_adam_schedule": (ctypes.c_int, [_DBL, ctypes.c_int64, ctypes.c_int64, ctypes.c_double, ctypes.c_double, _P]),
    "dudf_adam_step_scheduled": (ctypes.c_int, [_P, _P, _P, _P, ctypes.c_int64, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                                _P, ctypes.c_int64, _P, ctypes.c_double, _P]),
    "dudf_sample_batch_at": (ctypes.c_int, [_P, ctypes.c_int64, _P, _P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                            ctypes.c_int64, ctypes.c_uint64, _P, ctypes.c_int, ctypes.c_int, _P, _P, _P, _P]),
    "dudf_sample_batch": (ctypes.c_int, [_P, ctypes.c_int64, _P, _P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                         ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
                                         _P, _P, _P, _P]),
    "dudf_cloud_index_bytes": (ctypes.c_size_t, [ctypes.c_int64]),
    "dudf_cloud_morton_codes": (ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_size_t, _P, _P]),
    "dudf_cloud_index_build": (ctypes.c_int, [_P, ctypes.c_int64, _P, _P, ctypes.c_size_t, _P]),
    "dudf_sample_batch_indexed_at": (ctypes.c_int, [_P, ctypes.c_int64, _P, _P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                                    ctypes.c_int64, ctypes.c_uint64, _P, ctypes.c_int, ctypes.c_int,
                                                    _P, ctypes.c_size_t, _P, ctypes.c_size_t, _P, _P, _P, _P, _P]),
    "dudf_sample_batch_indexed": (ctypes.c_int, [_P, ctypes.c_int64, _P, _P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                                 ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
                                                 _P, ctypes.c_size_t, _P, ctypes.c_size_t, _P, _P, _P, _P, _P]),
    "dudf_capudf_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64]),
    "dudf_capudf_count": (ctypes.c_int, [_P, _P, ctypes.c_int64, ctypes.c_double, _P, _P, ctypes.c_size_t, _P]),
    "dudf_capudf_emit": (ctypes.c_int, [_P, _P, ctypes.c_int64, ctypes.c_double, _P, _P, _P, _P, ctypes.c_size_t, _P]),
    "dudf_grid_fields_lattice": (ctypes.c_int, [_CFG, _P, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
                                                ctypes.c_double, _P, _P, _P, _P, ctypes.c_size_t, _P]),
    "dudf_sparse_select_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int]),
    "dudf_sparse_select": (ctypes.c_int, [_P, ctypes.c_int64, ctypes.c_int, ctypes.c_double, _P, _P, _P, _P, _P, ctypes.c_size_t, _P]),
    "dudf_grid_fields_bricks": (ctypes.c_int, [_CFG, _P, ctypes.c_int64, ctypes.c_int, _P, ctypes.c_int64, ctypes.c_int, ctypes.c_double,
                                               _P, _P, _P, _P, ctypes.c_size_t, _P]),
    "dudf_capudf_sparse_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int, ctypes.c_int64]),
    "dudf_capudf_sparse_count": (ctypes.c_int, [_P, _P, _P, _P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_double, _P, _P,
                                                ctypes.c_size_t, _P]),
    "dudf_capudf_sparse_emit": (ctypes.c_int, [_P, _P, _P, _P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_double, _P, _P, _P,
                                               _P, ctypes.c_size_t, _P]),
    "dudf_grid_values": (ctypes.c_int, [_CFG, _P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, _P, _P, ctypes.c_size_t, _P]),
    "dudf_mc_lewiner_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64]),
    "dudf_mc_lewiner_count": (ctypes.c_int, [_P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_double, _P, _P, _P,
                                             ctypes.c_int, _P, _P, ctypes.c_size_t, _P]),
    "dudf_mc_lewiner_emit": (ctypes.c_int, [_P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_double, _P, _P, _P,
                                            ctypes.c_int, _P, _P, _P, _P, _P, ctypes.c_size_t, _P]),
    "dudf_mesh_clean_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int64]),
    "dudf_mesh_clean_count": (ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_int64, ctypes.c_int, ctypes.c_int, _P, _P, ctypes.c_size_t, _P]),
    "dudf_mesh_clean_emit": (ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_int64, ctypes.c_int, ctypes.c_int, _P, _P, _P,
                                            ctypes.c_size_t, _P]),
    "dudf_mesh_border_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int64]),
    "dudf_mesh_border_count": (ctypes.c_int, [ctypes.c_int64, _P, ctypes.c_int64, _P, _P, ctypes.c_size_t, _P]),
    "dudf_mesh_border_edges": (ctypes.c_int, [ctypes.c_int64, _P, ctypes.c_int64, _P, _P, ctypes.c_size_t, _P]),
    "dudf_mesh_smooth_borders": (ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_int64, ctypes.c_int, ctypes.c_double, _P,
                                                ctypes.c_size_t, _P]),
    "dudf_mesh_topology_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64]),
    "dudf_mesh_topology": (ctypes.c_int, [_P, ctypes.c_int64, ctypes.c_int64, _P, _P, _P, _P, _P, _P, _P, _P, ctypes.c_size_t, _P]),
    "dudf_mesh_submesh_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int64]),
    "dudf_mesh_submesh_count": (ctypes.c_int, [ctypes.c_int64, _P, ctypes.c_int64, _P, _P, _P, ctypes.c_size_t, _P]),
    "dudf_mesh_submesh_emit": (ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_int64, _P, _P, _P, _P, ctypes.c_size_t, _P]),
    "dudf_mesh_simplify_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int64]),
    "dudf_mesh_simplify_keys": (ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_int64, _DBL, ctypes.c_double, _P, _P, ctypes.c_size_t, _P]),
    "dudf_mesh_simplify_count": (ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_int64, _DBL, ctypes.c_double, ctypes.c_double,
                                                ctypes.c_double, _P, _P, ctypes.c_int, _P, _P, ctypes.c_size_t, _P]),
    "dudf_mesh_simplify_emit": (ctypes.c_int, [_P, ctypes.c_int64, _P, ctypes.c_int64, _P, _P, _P, _P, _P, _P, _P, _P, ctypes.c_size_t, _P]),
    "dudf_profile_enable": (ctypes.c_int, [ctypes.c_int]),
    "dudf_split_mode": (ctypes.c_int, []),
    "dudf_profile_dump": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_size_t]),
    "dudf_profile_clocks": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_size_t]),
    "dudf_profile_products": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_size_t]),
    "dudf_set_wgrad_max_workgroups": (ctypes.c_int, [ctypes.c_int]),
    "dudf_debug_read_stash": (ctypes.c_int, [_CFG, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                             ctypes.c_int64, _P, _P, ctypes.c_size_t, _P]),
    "dudf_debug_eigh3": (ctypes.c_int, [_P, ctypes.c_int64, _P, _P, _P]),
    "dudf_debug_loss_stage": (ctypes.c_int, [_CFG, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, _P, _P, _P, _P, _P, ctypes.c_int64,
                                             _DBL, ctypes.c_double, _P, _P, _P, _P, _P, _P, _P, _P, _P, ctypes.c_size_t, _P]),
    "dudf_debug_stash_layout": (ctypes.c_int, [_CFG, ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]),
    "dudf_debug_kernel_choice": (ctypes.c_int, [_CFG, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]),
    "dudf_stash_mode": (ctypes.c_int, [_CFG, ctypes.c_int64, ctypes.c_int64]),
    "dudf_set_option": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int]),
    "dudf_get_option": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]),
    "dudf_reset_options": (ctypes.c_int, []),
    "dudf_abi_version": (ctypes.c_int, []),
}
ABI_VERSION = 8          # DUDF_ABI_VERSION of include/dudf_hip.h this mirror was written against


def load():
    """Load libdudf_hip.so (built in-tree by `__graft_entry__.build()` / `make -C diffudf_amd/csrc`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DudfError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(hipcc --offload-arch=gfx950). There is no CPU fallback for the HIP path.")
    lib = ctypes.CDLL(LIB_PATH)
    try:
        lib.dudf_abi_version.restype = ctypes.c_int
        abi = int(lib.dudf_abi_version())
    except AttributeError:
        abi = None
    if abi != ABI_VERSION:                # a stale .so would read dudf_net_cfg / argument lists of another layout
        raise DudfError(f"{LIB_PATH} has ABI {abi}, this package binds ABI {ABI_VERSION}: rebuild it "
                        "(`python -c 'import __graft_entry__ as g; g.build()'`)")
    for name, (res, args) in SYMBOLS.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:           # calls added without an ABI bump (dudf_render_*, dudf_nearest_points, dudf_mesh_*, dudf_mc_lewiner_* ..: no existing signature changed)
            raise DudfError(f"{LIB_PATH} does not export {name}: it is older than this package; rebuild it "
                            "(`python -c 'import __graft_entry__ as g; g.build()'`)") from None
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what):
    if rc == 0:
        return
    if rc < 0:
        raise DudfError(f"{what}: {_ERRORS.get(rc, rc)}")
    raise DudfError(f"{what}: HIP error {rc}")
