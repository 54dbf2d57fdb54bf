# coding: utf-8
"""GPU: the fused march against a mesh (`dudf_mesh_trace_rays`, `MeshIndex.trace_rays`) against the reference loop
(src/render_st.py:255-268) restated in numpy with `MeshIndex.distance` as its distance query, and the mesh renderer on top of it
(`create_projectional_image_mesh`)."""
import os
import sys

import numpy as np
import pytest
import torch

import mesh_occupancy_oracle as OO
import meshdist_oracle as MO
from diffudf_amd import hip_ops, metrics, render_st

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAMERA, LIGHT, BOUND, EPS = [1.6, 1.2, 2.4], [2, 4, 8], 1.3, 0.001
# max over the hits of |normal - t0/|t0|| for the fp64 numpy composition of the same renderer (fp64 distances signed by the parity
# oracle, the same +-1e-4 stencil at the float32 positions) on the T = 320 icosphere with the rays of `scenes`: the facets are flat,
# so the figure is the angle between a facet's normal and the radial direction, not rounding.  Measured once, on the CPU.
SPHERE_NORMAL_ERROR_FP64 = 0.1801


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def numpy_march(scene, rays, t0, mask_rays, surface_eps, max_iterations, bound=BOUND):
    """The reference loop (tests/mesh_occupancy_oracle.py `march`) with `MeshIndex.distance` as its distance query."""
    return OO.march(lambda p: scene.distance(dev(p)).cpu().numpy(), rays, t0, mask_rays, surface_eps, max_iterations, bound)


@pytest.fixture(scope="module")
def scenes():
    """64 x 64 rays of generate_st's set-up against the T = 320 icosphere (120 degrees, so that part of them miss it) and against
    the beetle (the 45 degrees of configs/st_beetle_gt.json); the numpy march at 30 iterations, computed once."""
    import generate_st
    out = {}
    v, f = MO.bench_meshdist.icosphere(2)
    bv, bf, _ = MO.beetle()
    for name, (vv, ff, fov) in {"sphere": (v, f, 120), "beetle": (bv, bf, 45)}.items():
        scene = metrics.MeshIndex(vv, ff, device=DEV)
        rays, t0, mask = hip_ops.render_setup_rays(64, 64, fov, 0.5, generate_st.camera_rotation(CAMERA), CAMERA, [1, -1, 1, -1, 1, -1], DEV)
        r = {"scene": scene, "rays": rays.cpu().numpy(), "t0": t0.cpu().numpy(), "mask": mask.cpu().numpy().astype(bool)}
        w_t0, w_mask = r["t0"].copy(), r["mask"].copy()
        w_hits, fragile = numpy_march(scene, r["rays"], w_t0, w_mask, EPS, 30)
        r["want30"] = (w_t0, w_mask, w_hits, fragile)
        out[name] = r
    return out


def run_fused(s, rows, max_iterations, brute=False):
    t0, mask = dev(s["t0"][rows]), dev(s["mask"][rows].astype(np.uint8))
    hits = s["scene"].trace_rays(dev(s["rays"][rows]), t0, mask, surface_eps=EPS, max_iterations=max_iterations, bound=BOUND, brute=brute)
    assert hits.dtype == torch.uint8 and hits.shape == (len(rows),)
    return t0.cpu().numpy(), mask.cpu().numpy().astype(bool), hits.cpu().numpy().astype(bool)


def compare(got, want, label):
    (t0, mask, hits), (w_t0, w_mask, w_hits, fragile) = got, want
    keep = ~fragile
    err = np.abs(t0 - w_t0)[keep].max() if keep.any() else 0.0
    print(f"{label}: rays {len(hits)}, hits {int(w_hits.sum())}, alive {int(w_mask.sum())}, left out {int(fragile.sum())}, max |t0 - ref| {err:.3g}")
    assert fragile.sum() <= 0.005 * len(fragile)
    assert np.array_equal(hits[keep], w_hits[keep]) and np.array_equal(mask[keep], w_mask[keep])
    assert err <= 1e-12


@pytest.mark.parametrize("name", ["sphere", "beetle"])
def test_march_equals_the_numpy_loop(scenes, name):
    """One rounding per operation on both sides and the same distances: positions to 1e-12 (they come out equal), hits and masks
    identical.  Hits, misses (rays that leave the 1.3 box) and rays that never met the box are all present."""
    s = scenes[name]
    want = s["want30"]
    rows = np.arange(len(s["mask"]))
    compare(run_fused(s, rows, 30), want, name)
    assert 0 < want[2].sum() < s["mask"].sum() <= len(rows)
    t0, mask, hits = run_fused(s, rows, 30)
    assert not (hits & mask).any() and not (hits & ~s["mask"]).any()
    assert np.array_equal(t0[~s["mask"]], s["t0"][~s["mask"]])                # a ray that starts dead does not move


@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("max_iterations", [0, 1, 30])
def test_iteration_and_ray_counts(scenes, max_iterations, n):
    s = scenes["sphere"]
    step = max(1, int(s["mask"].sum()) // n)
    rows = np.flatnonzero(s["mask"])[step // 2:: step][:n]                             # spread over the image: the one ray hits, the 257 hit and miss
    assert len(rows) == n
    w_t0, w_mask = s["t0"][rows].copy(), s["mask"][rows].copy()
    w_hits, fragile = numpy_march(s["scene"], s["rays"][rows], w_t0, w_mask, EPS, max_iterations)
    got = run_fused(s, rows, max_iterations)
    compare(got, (w_t0, w_mask, w_hits, fragile), f"sphere n={n} iterations={max_iterations}")
    if max_iterations == 0:
        assert np.array_equal(got[0], s["t0"][rows]) and got[1].all() and not got[2].any()
    b = run_fused(s, rows, max_iterations, brute=True)                                  # without the index: the same bits
    assert np.array_equal(b[0], got[0]) and np.array_equal(b[1], got[1]) and np.array_equal(b[2], got[2])


def test_all_miss_raises(scenes):
    s = scenes["sphere"]
    n = 16
    rays = np.tile(np.array([[1.0, 0.0, 0.0]]), (n, 1))
    t0 = np.tile(np.array([[1.1, 0.0, 0.0]]), (n, 1)); t0[:, 1] = np.linspace(-0.5, 0.5, n)
    mask = np.ones(n, dtype=bool)
    with pytest.raises(ValueError, match="Ray tracing did not converge in 30 iterations to any point at distance 0.001 or lower"):
        render_st.create_projectional_image_mesh(s["scene"], 4, 4, rays, t0, mask, LIGHT, device=DEV)
    assert not mask.any() and (t0[:, 0] >= BOUND).all()                                 # in place, as the reference leaves them
    with pytest.raises(render_st.DudfError):
        s["scene"].trace_rays(torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4, 3, dtype=torch.float64), torch.ones(4, dtype=torch.uint8))


def test_sphere_normals_and_image(scenes):
    """On the sphere the rendered normals point along t0/|t0| as well as the stencil on a faceted sphere allows:
    SPHERE_NORMAL_ERROR_FP64 = 0.1801 is that error for the fp64 numpy composition (the facets, not rounding); the device's
    float32 distances must stay within twice that.  The image: 0.2 .. 0.9 grey at the hits, 1.0 elsewhere."""
    s = scenes["sphere"]
    w_t0, w_mask, w_hits, fragile = s["want30"]
    d_t0, d_hits, d_rays = dev(w_t0), dev(w_hits.astype(np.uint8)), dev(s["rays"])
    pos, hit_rays, rows, k = hip_ops.render_gather(d_hits, d_t0, d_rays)
    normals = render_st.mesh_normals(s["scene"], pos, hit_rays).cpu().numpy()
    p = pos.cpu().numpy()
    radial = p / np.linalg.norm(p, axis=1, keepdims=True)
    err = np.linalg.norm(normals - radial, axis=1)
    print(f"sphere normals: {k} hits, max |n - t0/|t0|| {err.max():.4f}, median {np.median(err):.4f}; fp64 composition {SPHERE_NORMAL_ERROR_FP64}")
    assert k == w_hits.sum() and np.abs(np.linalg.norm(normals, axis=1) - 1).max() < 1e-6
    assert err.max() <= 2 * SPHERE_NORMAL_ERROR_FP64
    assert ((normals * s["rays"][w_hits]).sum(axis=1) <= 0).all()                      # oriented against the rays
    t0, mask = s["t0"].copy(), s["mask"].copy()
    img = render_st.create_projectional_image_mesh(s["scene"], 64, 64, s["rays"], t0, mask, LIGHT, device=DEV)
    assert img.shape == (64, 64, 3) and img.dtype == np.float64
    flat = img.reshape(-1, 3)
    keep = ~fragile
    assert (flat[~w_hits & keep] == 1.0).all() and (flat[w_hits & keep] <= 0.9).all() and (flat[w_hits & keep] >= 0.2 - 1e-12).all()
    assert np.abs(t0 - w_t0)[keep].max() <= 1e-12 and np.array_equal(mask[keep], w_mask[keep])


def test_fused_march_is_not_slower_than_the_composed_loop():
    """tools/bench_meshtrace.py's own timer and composed loop (`MeshIndex.distance` + torch masking per iteration) at 128 x 128
    rays on the T = 20 480 icosphere; the composed loop pays ~30 launches of the walker, the compaction and a host read per
    iteration, so only ratio > 1 is asserted."""
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import bench_meshtrace
    r = bench_meshtrace.measure(size=128, level=5, reps=5, warmup=1, parts=("sphere",))
    print("bench_meshtrace:", r)
    assert r["sphere"]["rays"] == 16384 and r["sphere"]["triangles"] == 20480 and r["sphere"]["same_result"]
    assert r["sphere"]["ratio_composed_over_fused"] > 1
