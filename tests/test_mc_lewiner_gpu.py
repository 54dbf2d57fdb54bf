# coding: utf-8
"""GPU: Lewiner marching cubes of a signed volume on the device (csrc/dudf_mcsdf.hip) against the host library
(`dudf_mc_lewiner_run`, held by tests/test_mc_lewiner_cpu.py): the same bits in the same order — vertices, faces, normal sums,
unit normals, values —, and `get_mesh_sdf` / `generate_mc(..., algorithm='siren')` on top of it."""
import os
import time

import numpy as np
import pytest
import torch

from diffudf_amd import marching_cubes as M

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def luts():
    z = np.load(os.path.join(HERE, "golden", "g10_meshudf.npz"))
    return {k[4:]: z[k] for k in z.files if k.startswith("lut_")}


def both(vol, level, luts, raw=True):
    host = M.marching_cubes_sdf(vol, level, luts, raw_normals=raw)
    dev = M.marching_cubes_sdf(torch.from_numpy(vol).cuda(), level, luts, raw_normals=raw)
    return host, [t.cpu().numpy() for t in dev]


def assert_same(host, dev, what):
    for name, h, d in zip(("vertices", "faces", "normals", "values"), host, dev):
        assert h.dtype == d.dtype and h.shape == d.shape, (what, name, h.shape, d.shape)
        assert np.array_equal(h, d), (what, name, int((h != d).sum()))


def uses_centre_vertex(vol, level, luts):
    """The host run met a tiling with edge 12: some vertex lies strictly inside a cube."""
    v = M.marching_cubes_sdf(vol, level, luts)[0]
    return bool(((v != np.floor(v)).sum(axis=1) == 3).any())


@pytest.mark.parametrize("shape", [(2, 2, 2), (3, 2, 5), (9, 10, 11), (17, 33, 65), (70, 70, 70)])
def test_noise_volumes_bit_for_bit(luts, shape):
    # (9, 10, 11) and (70, 70, 70): rows of 10 / 69 cells, so 256-cell workgroups end mid-row; (17, 33, 65): several workgroups of
    # whole rows; (70, 70, 70): 328 509 cells = 1284 workgroups, so the scan's 1024 threads take more than one workgroup each
    vol = np.random.default_rng(sum(shape)).normal(size=shape).astype(np.float32)
    host, dev = both(vol, 0.0, luts)
    assert len(host[0]) > 0
    if min(shape) >= 9:
        assert uses_centre_vertex(vol, 0.0, luts)
    assert_same(host, dev, shape)
    host_u, dev_u = both(vol, 0.0, luts, raw=False)                      # unit normals: the wrapper's own arithmetic on either side
    assert_same(host_u, dev_u, shape)


def test_sphere_at_a_level(luts):
    g = np.meshgrid(*[np.arange(48, dtype=np.float64)] * 3, indexing="ij")
    vol = (np.sqrt((g[0] - 21.3) ** 2 + (g[1] - 25.9) ** 2 + (g[2] - 22.6) ** 2) / 16.0 - 1.0).astype(np.float32)
    host, dev = both(vol, 0.1, luts)
    assert len(host[0]) > 1000
    assert_same(host, dev, "sphere")
    hv, hf, hn, _ = M.marching_cubes_lewiner(vol, 0.1, spacing=(0.5, 0.25, 2.0), luts=luts)
    dv, df, dn, _ = M.marching_cubes_lewiner(torch.from_numpy(vol).cuda(), 0.1, spacing=(0.5, 0.25, 2.0), luts=luts)
    assert dv.dtype == torch.float64 and df.dtype == torch.int32
    assert np.array_equal(hv, dv.cpu().numpy()) and np.array_equal(hf, df.cpu().numpy()) and np.array_equal(hn, dn.cpu().numpy())


def test_values_equal_to_the_level(luts):
    vol = (np.arange(7, dtype=np.float32)[:, None, None] - 3.0 + np.zeros((7, 5, 6), np.float32))
    vol[2:5, 1:3, 2:4] = 0.0                                            # a block of exact zeros inside as well
    host, dev = both(vol, 0.0, luts)
    assert len(host[0]) > 0
    assert_same(host, dev, "integer field")


def test_nothing_to_extract(luts):
    from diffudf_amd import hip_ops
    vol = torch.ones(5, 6, 7, device="cuda")
    data, offs, dims = M._pack_luts(luts)
    launched = []
    real = hip_ops._call

    def spy(name, *a, **k):
        launched.append(name)
        return real(name, *a, **k)
    hip_ops._call = spy
    try:
        v, f, n, vals = hip_ops.mc_lewiner_extract(vol, 1.0, torch.from_numpy(data).cuda(), offs, dims)
    finally:
        hip_ops._call = real
    assert v.shape == (0, 3) and f.shape == (0, 3) and n.shape == (0, 3) and vals.shape == (0,)
    assert launched == ["dudf_mc_lewiner_count"]                        # counts (0, 0): the emit launch is not made
    with pytest.raises(RuntimeError, match="No surface found"):
        M.marching_cubes_lewiner(vol, 1.0, luts=luts)                    # in range, and nothing lies above it
    with pytest.raises(ValueError, match="within volume data range"):
        M.marching_cubes_lewiner(vol, 2.0, luts=luts)


def test_two_launches_give_the_same_bytes(luts):
    vol = torch.from_numpy(np.random.default_rng(3).normal(size=(21, 22, 23)).astype(np.float32)).cuda()
    a = M.marching_cubes_sdf(vol, 0.0, luts, raw_normals=True)
    b = M.marching_cubes_sdf(vol, 0.0, luts, raw_normals=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y) and x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


def small_siren():
    from diffudf_amd import synth
    from diffudf_amd.model import SIREN
    hidden = [64, 64]
    P = synth.siren_params(hidden, seed=7)
    m = SIREN(3, 1, hidden, w0=30).cuda()
    with torch.no_grad():
        m.flat_parameters().copy_(torch.from_numpy(synth.flatten_params(P)).cuda())
    return m, [(w.astype(np.float64), b.astype(np.float64)) for w, b in P]


def test_get_mesh_sdf(luts, tmp_path):
    from diffudf_amd import render_mc
    from oracle import dudf_oracle as O
    N = 24
    model, P64 = small_siren()
    vals = render_mc.sdf_grid_values(model, N, "cuda:0", max_batch=5000)          # ragged chunks
    x = np.linspace(-1.0, 1.0, N)
    voxel = 2.0 / (N - 1)
    idx = np.arange(N, dtype=np.float32)
    x32 = (idx * np.float32(voxel) - np.float32(1.0)).astype(np.float64)          # the coordinates the kernel derives from the index
    Z, Y, X = np.meshgrid(x32, x32, x32, indexing="ij")
    want, _ = O.forward(P64, np.stack([Z.ravel(), Y.ravel(), X.ravel()], 1))
    got = vals.cpu().numpy().astype(np.float64).ravel()
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"grid values vs fp64 oracle: {err:.2e} relative to the max-norm")
    assert err < 5e-6                                                              # the value tolerance of tests/test_hip_parity.py
    assert want.min() < 0 < want.max()
    assert np.abs(x - x32).max() < 1e-6
    offset, scale = np.array([0.1, -0.2, 0.3]), 1.7
    verts, faces, mesh = render_mc.get_mesh_sdf(model, N=N, device="cuda:0", max_batch=5000, offset=offset, scale=scale, luts=luts)
    hv, hf, hn, _ = M.marching_cubes_lewiner(vals.cpu().numpy(), 0.0, spacing=[voxel] * 3, luts=luts)
    assert len(hf) > 0
    assert np.array_equal(verts, (hv - 1.0) / scale - offset) and np.array_equal(faces, hf)
    assert np.array_equal(np.asarray(mesh.faces), hf) and np.array_equal(np.asarray(mesh.vertex_normals, np.float32), hn)
    # generate_mc(..., algorithm='siren') from a checkpoint file, as train.py calls it
    from generate_mc import generate_mc
    ckpt, out = str(tmp_path / "model.pth"), str(tmp_path / "mesh.obj")
    torch.save(model.state_dict(), ckpt)
    generate_mc(None, "siren", 0, N, out, algorithm="siren", luts=luts,
                from_file={"w0": 30, "model_path": ckpt, "hidden_layer_nodes": [64, 64]})
    assert os.path.getsize(out) > 0


def test_device_beats_the_host_library(luts):
    N = 128
    g = torch.arange(N, device="cuda", dtype=torch.float32)
    vol = (torch.sqrt((g[:, None, None] - 61.3) ** 2 + (g[None, :, None] - 66.1) ** 2 + (g[None, None, :] - 63.7) ** 2) - 45.0).contiguous()
    host_vol = vol.cpu().numpy()
    M.marching_cubes_sdf(vol, 0.0, luts)                                           # warm both sides
    M.marching_cubes_sdf(host_vol, 0.0, luts)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dev = M.marching_cubes_sdf(vol, 0.0, luts)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    host = M.marching_cubes_sdf(host_vol, 0.0, luts)
    t2 = time.perf_counter()
    assert dev[0].shape == host[0].shape
    ratio = (t2 - t1) / (t1 - t0)
    print(f"128^3 sphere: host library {1e3 * (t2 - t1):.2f} ms, device {1e3 * (t1 - t0):.2f} ms, ratio {ratio:.1f}")
    assert ratio > 1
