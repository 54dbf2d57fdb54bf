# coding: utf-8
"""CPU: the point-cloud entry points exist behind the reference's names (reference src/render_pc.py:10-26, generate_pc.py:6),
the PLY fallback round-trips, the round workspace size is host arithmetic, and the fixture's own margin holds."""
import ctypes
import inspect
import os

import numpy as np
import pytest

from diffudf_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
G14 = os.path.join(HERE, "golden", "g14_pointcloud.npz")


def test_sampler_has_the_reference_signatures():
    from src.render_pc import Sampler
    p = inspect.signature(Sampler.__init__).parameters
    assert list(p)[1:] == ["n_in_features", "hidden_layers", "w0", "ww", "checkpoint", "device"]
    assert [p[k].default for k in list(p)[1:]] == [3, [256, 256, 256, 256], 30, None, None, 0]
    g = inspect.signature(Sampler.generate_point_cloud).parameters
    names = list(g)[1:]
    assert names[:6] == ["gt_mode", "alpha", "num_steps", "num_points", "surf_thresh", "max_iter"]
    assert [g[k].default for k in ("num_steps", "num_points", "surf_thresh", "max_iter")] == [5, 20000, 0.01, 1000]
    assert g["gt_mode"].default is inspect.Parameter.empty and g["alpha"].default is inspect.Parameter.empty
    extra = {k: g[k] for k in names[6:]}
    assert {k: v.default for k, v in extra.items()} == {"rng": "numpy", "seed": None, "check_every": 8, "return_tensors": False}
    assert all(v.kind is inspect.Parameter.KEYWORD_ONLY for v in extra.values())
    assert hasattr(Sampler, "from_model")


def test_generate_pc_entry_point():
    import generate_pc
    assert list(inspect.signature(generate_pc.generate_pc).parameters) == ["config"]


def test_ply_fallback_round_trips(tmp_path):
    import generate_pc
    from diffudf_amd.mesh import read_ply_points
    rng = np.random.default_rng(3)
    pos = rng.uniform(-1, 1, (1001, 3)); nrm = rng.normal(size=(1001, 3))
    path = str(tmp_path / "cloud.ply")
    generate_pc.PointCloud(pos, nrm).write(path)
    with open(path, "rb") as f:
        head = f.read(64)
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex 1001\n")
    p, n = read_ply_points(path)
    assert np.array_equal(p, pos.astype(np.float32)) and np.array_equal(n, nrm.astype(np.float32))
    generate_pc.PointCloud(np.zeros((0, 3)), np.zeros((0, 3))).write(path)          # an empty cloud is a valid file
    p, n = read_ply_points(path)
    assert p.shape == (0, 3) and n.shape == (0, 3)


def test_round_workspace_is_host_arithmetic():
    lib = _lib.load()
    cfg = _lib.NetCfg(3, 8, 256, 30.0)
    q = lib.dudf_workspace_bytes_query(ctypes.byref(cfg), 20000, 0)
    nb = lib.dudf_pointcloud_workspace_bytes(ctypes.byref(cfg), 20000)
    # the value+gradient query layout, the float64 samples / proposals / unit gradients, two float32 position arrays, and a
    # frame-query layout for one chunk of accepted rows
    assert nb >= q + 20000 * (3 * 24 + 2 * 12 + 1) + lib.dudf_workspace_bytes_query(ctypes.byref(cfg), 20000, 20000)
    assert nb % 256 == 0
    big = lib.dudf_pointcloud_workspace_bytes(ctypes.byref(cfg), 1000000)
    assert big < lib.dudf_workspace_bytes_query(ctypes.byref(cfg), 1000000, 0) + (8 << 30)   # the Hessian part is chunked
    assert lib.dudf_pointcloud_workspace_bytes(ctypes.byref(cfg), 0) > 0
    assert lib.dudf_pointcloud_workspace_bytes(ctypes.byref(_lib.NetCfg(3, 8, 100, 30.0)), 20000) == 0
    assert lib.dudf_pointcloud_workspace_bytes(ctypes.byref(cfg), -1) == 0
    assert lib.dudf_pointcloud_append_workspace_bytes(1000003) >= 2 * 4 * ((1000003 + 255) // 256)
    assert lib.dudf_abi_version() == 8 == _lib.ABI_VERSION


def test_cpu_tensors_are_refused():
    import torch
    from diffudf_amd import hip_ops
    cfg = hip_ops.make_cfg([32, 32])
    with pytest.raises(_lib.DudfError):
        hip_ops.project_points(cfg, torch.zeros(1), torch.zeros(4, 3, dtype=torch.float64), "tanh", 100.0)


def test_fixture_margin():
    """The allowance the GPU test grants (accept flags equal on >= 99 % of the points) must be one the reference alone meets:
    its float32 and float64 runs agree on >= 99.5 %."""
    g = np.load(G14)
    for net in ("t", "s"):
        for mode in ("tanh", "siren"):
            assert float(g[f"{net}_{mode}_fate"]) >= 0.995
    assert float(g["e2e_d_ref"]) > 0 and 0 < float(g["e2e_c_ref"]) <= 1
