# coding: utf-8
"""GPU: the device surface sampler (`metrics.sample_surface`, csrc/dudf_surfsample.hip) against the numpy oracle of
tests/surface_oracle.py (pinned by tests/test_surface_oracle_cpu.py).  Points, normals, faces and face normals are compared bit for
bit: the kernel and the oracle evaluate the same fp64 expressions in the same order and choose faces by integer arithmetic.  The
area is a sum in another order than the oracle's `math.fsum`: 1e-13 relative (F <= 262 149 additions of round-off 1.1e-16 each, in
a tree: the error grows like log2 F, not like F)."""
import os

import numpy as np
import pytest
import torch

import surface_oracle as SO
from diffudf_amd import mesh, metrics
from diffudf_amd._lib import DudfError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
BIG_F = 256 * 1024 + 5            # 1 025 workgroups of 256 faces: the scan of totals gives two totals to a thread
BIG_N = 4096 * 256 + 300          # more samples than the capped grid has threads: the kernel strides


def _grid(F, nx, ny):
    """The first F faces of a planar grid whose face areas range over 6 decades, a few of them degenerate."""
    v, f = SO.planar_grid(nx, ny, decades=6.0, degenerate=[d for d in (0, 3, 100, 254, 255, 256, 70000, BIG_F - 1) if d < F])
    assert len(f) >= F
    return v, np.ascontiguousarray(f[:F])


@pytest.fixture(scope="module")
def meshes():
    bv, bt = mesh.load_obj(os.path.join(HERE, "golden", "beetle.obj"))
    out = {1: (np.array([[0.1, 0.2, 0.3], [1.0, 0.0, 0.5], [0.0, 1.0, -0.5]]), np.array([[0, 1, 2]], dtype=np.int64)),
           2: (np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [4, 0, 0]]), np.array([[0, 1, 2], [1, 3, 2]], dtype=np.int64)),   # areas 0.5, 1.5
           2053: (mesh.normalize_vertices(bv), bt)}
    for F in (255, 256, 257):
        out[F] = _grid(F, 16, 9)
    out[BIG_F] = _grid(BIG_F, 512, 257)
    assert len(bt) == 2053
    nn = SO.face_terms(*out[BIG_F])[1]
    assert nn[nn > 0].max() / nn[nn > 0].min() > 1e5 and (nn == 0).sum() >= 5
    return out


def _device_sample(v, f, n, **kw):
    p, nm, face = metrics.sample_surface(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV), n, return_face=True, **kw)
    assert p.dtype == torch.float32 and nm.dtype == torch.float32 and face.dtype == torch.int64
    assert p.shape == (n, 3) and nm.shape == (n, 3) and face.shape == (n,)
    return p.cpu().numpy(), nm.cpu().numpy(), face.cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("F,n", [(1, 1), (2, 255), (255, 256), (256, 257), (257, 255), (2053, 257), (2053, BIG_N), (BIG_F, 1),
                                 (BIG_F, BIG_N)])
def test_kernel_against_oracle(meshes, F, n):
    v, f = meshes[F]
    want_p, want_n, want_face, want_fn, want_area = SO.sample_surface(v, f, n, seed=123)
    p, nm, face = _device_sample(v, f, n, seed=123)
    assert np.array_equal(face, want_face)
    assert _same_bits(p, want_p) and _same_bits(nm, want_n)
    fn = metrics.face_normals(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV))
    assert fn.dtype == torch.float32 and _same_bits(fn.cpu().numpy(), want_fn)
    area = metrics.surface_area(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV))
    assert isinstance(area, float) and abs(area - want_area) <= 1e-13 * want_area
    nn = SO.face_terms(v, f)[1]
    assert (nn[face] > 0).all()                                  # no degenerate face was chosen


def test_numpy_inputs_are_uploaded(meshes):
    v, f = meshes[2053]
    p, nm = metrics.sample_surface(v, f, 300, seed=4)
    assert p.device.type == "cuda"
    want = SO.sample_surface(v, f, 300, seed=4)
    assert _same_bits(p.cpu().numpy(), want[0]) and _same_bits(nm.cpu().numpy(), want[1])
    # a float32 mesh is converted, not refused: the samples are those of its exact double values
    p32, _ = metrics.sample_surface(torch.from_numpy(v.astype(np.float32)).to(DEV), torch.from_numpy(f.astype(np.int32)).to(DEV), 300, seed=4)
    assert _same_bits(p32.cpu().numpy(), SO.sample_surface(v.astype(np.float32).astype(np.float64), f, 300, seed=4)[0])


def test_planted_uniforms():
    # the mesh of test_weight_zero_face_is_never_chosen: c = [2^32, 2^32, 2^33, 2^33, 3 * 2^32]
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [2.0 ** -34, 0, 0], [0, 0, 1]], dtype=np.float64)
    f = np.array([[0, 1, 2], [1, 3, 3], [1, 3, 2], [0, 4, 2], [0, 1, 5]], dtype=np.int64)
    last = 1.0 - 2.0 ** -53
    u = np.array([[0.0, 0.5, 0.5],                               # u1 = 0
                  [last, 0.5, 0.5],                              # the largest double below 1: the last face
                  [3002399751580330 / SO.TWO53, 0.3, 0.6],       # t = 2^32 - 1: still face 0
                  [3002399751580331 / SO.TWO53, 0.3, 0.6],       # t = 2^32 = c_0 = c_1 exactly: side="right" skips the empty face 1
                  [6004799503160662 / SO.TWO53, 0.3, 0.6],       # t = 2^33 = c_2 = c_3 exactly: face 4
                  [0.5, 0.0, 0.7],                               # r1 = 0: vertex A of the face
                  [0.5, last, 0.0],                              # r2 = 0: on the edge A B
                  [0.9, last, last]])
    assert [(int(k) * 3 * 2 ** 32) >> 53 for k in np.floor(u[:, 0] * SO.TWO53)][2:5] == [2 ** 32 - 1, 2 ** 32, 2 ** 33]
    want = SO.sample_surface(v, f, len(u), uniforms=u)
    assert want[2].tolist() == [0, 4, 0, 2, 4, 2, 2, 4]
    p, nm, face = _device_sample(v, f, len(u), uniforms=torch.from_numpy(u).to(DEV))
    assert face.tolist() == want[2].tolist() and _same_bits(p, want[0]) and _same_bits(nm, want[1])
    assert p[5].tolist() == [1.0, 0.0, 0.0]                      # A of face 2
    assert p[6, 2] == 0.0 and p[6, 0] == 1.0 and p[6, 1] > 0.0   # on the edge from A = (1, 0, 0) to B = (1, 1, 0)
    for bad in (1.0, -2.0 ** -60, float("nan"), float("inf")):
        for col in range(3):
            w = u.copy(); w[3, col] = bad
            with pytest.raises(ValueError):
                metrics.sample_surface(v, f, len(u), uniforms=w)


def test_split_seed_and_repeat(meshes):
    v, f = meshes[2053]
    whole = _device_sample(v, f, 1000, seed=77)
    head, tail = _device_sample(v, f, 400, seed=77), _device_sample(v, f, 600, seed=77, start=400)
    for k in range(3):
        assert np.array_equal(whole[k].view(np.uint32 if k < 2 else np.int64), np.concatenate([head[k], tail[k]]).view(np.uint32 if k < 2 else np.int64))
    again = _device_sample(v, f, 1000, seed=77)
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(whole, again))
    other = _device_sample(v, f, 1000, seed=78)
    assert (other[2] != whole[2]).mean() > 0.9 and not np.array_equal(other[0], whole[0])
    assert _device_sample(v, f, 0, seed=77)[0].shape == (0, 3)


def test_area_shares(meshes):
    """Two triangles of areas 1 : 3: the larger one's share of n = 40 000 samples is binomial, sigma = sqrt(0.75 * 0.25 / n)."""
    v, f = meshes[2]
    n = 40000
    face = _device_sample(v, f, n, seed=2024)[2]
    assert abs((face == 1).mean() - 0.75) <= 4.0 * np.sqrt(0.75 * 0.25 / n)


def test_errors(meshes):
    v, f = meshes[2]
    dv, df = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
    with pytest.raises(DudfError):                               # F = 0
        metrics.sample_surface(dv, df[:0], 10)
    with pytest.raises(DudfError, match="degenerate"):           # collinear and collapsed faces only
        metrics.sample_surface(torch.tensor([[0.0, 0, 0], [1, 0, 0], [2, 0, 0]], dtype=torch.float64, device=DEV),
                               torch.tensor([[0, 1, 2], [0, 0, 1]], device=DEV), 10)
    bad = dv.clone(); bad[3, 1] = float("nan")
    with pytest.raises(ValueError):
        metrics.sample_surface(bad, df, 10)
    with pytest.raises(DudfError, match="GPU"):                  # CPU tensors: no fallback
        metrics.sample_surface(torch.from_numpy(v), torch.from_numpy(f), 10)
    for wrong in (4, -1):
        g = df.clone(); g[1, 2] = wrong
        with pytest.raises(ValueError):
            metrics.sample_surface(dv, g, 10)
    with pytest.raises(DudfError):
        metrics.sample_surface(dv, df, -1)
    with pytest.raises(DudfError):
        metrics.surface_area(dv, df[:0])
    # the device is fine afterwards
    assert metrics.surface_area(dv, df) == pytest.approx(2.0, rel=1e-15)
