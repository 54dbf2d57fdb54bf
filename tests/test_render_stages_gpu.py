# coding: utf-8
"""GPU: the image stages of generate_st around the march (csrc/dudf_render.hip: ray set-up, gather, orientation, colour map,
shading with the scatter, 8-bit finish) and `hip_ops.render_percentile_bounds` against the numpy oracle of tests/render_oracle.py
(pinned to the reference's own run by tests/test_render_oracle_cpu.py), at the row counts where a 256-wide workgroup or the
4096-workgroup grid cap changes what a thread does, and on planted rows that sit on every comparison the kernels make.
Each test prints what it measures before it asserts."""
import functools
import os
import zlib

import numpy as np
import pytest
import torch

import generate_st
import render_oracle as RO
from diffudf_amd import hip_ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BIG = 4096 * 256 + 300                 # past one trip of every grid-stride loop (4096 workgroups of 256)
SMALL = (1, 255, 256, 257)
ROWS = SMALL + (BIG,)


def _cuda(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)              # a copy: the cached inputs are read-only


def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()))


# ---- ray set-up ------------------------------------------------------------------------------------------------------------------
GRIDS = [(1, 1), (5, 3), (3, 5), (16, 17), (257, 1), (1025, 1025)]
DEFAULT = (1, -1, 1, -1, 1, -1)


def camera(name, w, h):
    """(fov, noise, position, planes).  'axis': on +z with the pixel centres unjittered, so that the middle column (odd width) or
    row (odd height) has a ray component of exactly 0 and the parallel-plane branch runs.  'miss': jittered by two image sizes
    off to one side under a wide lens: every ray passes the box at more than 57 degrees off the axis, the box spans 37.
    'planes': the oblique camera against a smaller box."""
    return {"oblique": (45, 0.39068503, [0.8939, 0.7, 2.86], DEFAULT),
            "axis": (45, 0.5, [0, 0, 2.9], DEFAULT),
            "inside": (60, 0.3, [0.2, -0.1, 0.3], DEFAULT),
            "miss": (120, 2.0 * max(w, h), [0, 0, 2.9], DEFAULT),
            "planes": (45, 0.61874965, [0.8939, 0.7, 2.86], (0.5, -0.5, 0.8, -0.75, 1, -0.25))}[name]


# Rays whose smallest decision margin in the ORACLE is below 1e-9, counted on the CPU: 0 in each of the 30 cases, so the mask is
# compared on every ray.  The smallest margin of all is 2.5e-8 ('inside', 1025x1025; 'planes' 4.8e-8, 'oblique' 8.1e-7 there); a
# ray component of exactly 0 ('axis': 1, 7, 7, 16, 257 and 2049 rays of the six grids) is 1e-5 away from its threshold.
@pytest.mark.parametrize("name", ["oblique", "axis", "inside", "miss", "planes"])
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_setup(grid, name):
    """rays and t0 within 1e-12 (the bound of test_render_gpu.py::test_ray_setup), mask equal wherever the oracle's own decision
    margin exceeds 1e-9; rays below that margin: at most 0.1 % of the case."""
    w, h = grid
    fov, noise, pos, planes = camera(name, w, h)
    R = generate_st.camera_rotation(pos)
    rays, t0, mask = hip_ops.render_setup_rays(w, h, fov, noise, R, pos, planes, DEV)
    rays, t0, mask = rays.cpu().numpy(), t0.cpu().numpy(), mask.cpu().numpy()
    wr, wt, wm, margin = RO.setup_rays(w, h, fov, noise, R, pos, planes)
    sure = margin > 1e-9
    unsure = int((~sure).sum())
    er = np.abs(rays - wr).max()
    et = np.abs(t0[sure] - wt[sure]).max() if sure.any() else 0.0
    print(f"set-up {name} {w}x{h}: max |rays - oracle| {er:.3e}, max |t0 - oracle| {et:.3e}, valid {int(wm.sum())} of {w * h}, "
          f"{unsure} rays with a margin below 1e-9 (smallest {margin.min():.3e}), zero components {int((wr == 0).any(1).sum())}")
    assert rays.shape == t0.shape == (w * h, 3) and mask.dtype == np.uint8 and set(np.unique(mask)) <= {0, 1}
    assert unsure <= 1e-3 * w * h
    assert np.isfinite(wt).all() and np.isfinite(t0).all()
    assert np.array_equal(mask[sure].astype(bool), wm[sure])
    assert er <= 1e-12 and et <= 1e-12
    assert np.all(t0[mask == 0] == 0.0)
    if name == "miss":
        assert not mask.any() and not t0.any()
    else:
        assert wm.any()
    if name == "axis" and (w % 2 or h % 2):
        assert (wr == 0).any() and np.array_equal(rays == 0, wr == 0)            # the |den| < 1e-5 branch did run, on the same rays
    if name == "inside":
        assert wm.all()


# ---- gather ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 257, 70001])
@pytest.mark.parametrize("kind", ["none", "all", "random"])
def test_gather(m, kind):
    rng = _rng("gather", m, kind)
    hits = {"none": np.zeros(m, bool), "all": np.ones(m, bool), "random": rng.rand(m) < 0.4}[kind]
    t0, rays = rng.standard_normal((m, 3)), rng.standard_normal((m, 3))
    pos, hr, rows, k = hip_ops.render_gather(_cuda(hits.astype(np.uint8)), _cuda(t0), _cuda(rays))
    wp, wr, wrows, wk = RO.gather(hits, t0, rays)
    print(f"gather m = {m}, {kind}: k = {k} (oracle {wk})")
    assert k == wk and tuple(pos.shape) == (k, 3) and tuple(hr.shape) == (k, 3) and tuple(rows.shape) == (k,)
    assert rows.dtype == torch.int32 and np.array_equal(rows.cpu().numpy(), wrows)
    assert pos.cpu().numpy().tobytes() == wp.tobytes() and hr.cpu().numpy().tobytes() == wr.tobytes()
    pos2, none, rows2, k2 = hip_ops.render_gather(_cuda(hits.astype(np.uint8)), _cuda(t0))       # without the rays
    assert none is None and k2 == wk and np.array_equal(rows2.cpu().numpy(), wrows) and pos2.cpu().numpy().tobytes() == wp.tobytes()


# ---- orientation -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _frames(k):
    """k random right-handed orthonormal float32 frames (columns v0, v1, v2), unit float64 rays, float32 mean curvatures; planted
    from the front as far as k allows: n . ray == 0 exactly, a NaN frame, a third column of length 3, n . ray the smallest positive double."""
    rng = _rng("frames", k)
    a, b = rng.standard_normal((k, 3)), rng.standard_normal((k, 3))
    v2 = a / np.linalg.norm(a, axis=1)[:, None]
    v0 = np.cross(v2, b); v0 /= np.linalg.norm(v0, axis=1)[:, None]
    V = np.stack([v0, np.cross(v2, v0), v2], axis=2).astype(np.float32)
    rays = rng.standard_normal((k, 3)); rays /= np.linalg.norm(rays, axis=1)[:, None]
    mean = (rng.standard_normal(k) * 7).astype(np.float32)
    planted = [(np.float32([[1, 0, 0], [0, 1, 0], [0, 0, 1]]), [1.0, 0, 0]),
               (np.full((3, 3), np.nan, np.float32), [0, 1.0, 0]),
               (np.float32([[1, 0, 0], [0, 1, 0], [0, 0, 3]]), [0, 0.6, 0.8]),
               (np.float32([[1, 0, 0], [0, 1, 0], [0, 0, 1]]), [0, 1.0, 5e-324])]
    for i, (f, r) in enumerate(planted[:k]):
        V[i], rays[i] = f, r
    for a_ in (V, rays, mean):
        a_.setflags(write=False)
    return V, rays, mean


@pytest.mark.parametrize("k", ROWS)
def test_orient_frames(k):
    V, rays, mean = _frames(k)
    wn, w1, w2, wmean = RO.orient_frame(V, rays, mean)
    dmean = _cuda(mean.copy())
    n, pc1, pc2 = hip_ops.render_orient(_cuda(rays), frame_v=_cuda(V), mean=dmean, want_pc=True)
    n, pc1, pc2, dmean = n.cpu().numpy(), pc1.cpu().numpy(), pc2.cpu().numpy(), dmean.cpu().numpy()
    flipped = int((wn[:, 2] != V[:, 2, 2]).sum())
    print(f"orient k = {k}: {flipped} normals turned, {int((wn == 0).all(1).sum())} zeroed (n . ray == 0), {int(np.isnan(wn).any(1).sum())} NaN")
    assert n.dtype == np.float64 and dmean.dtype == np.float32
    assert np.array_equal(n, wn, equal_nan=True)
    assert np.array_equal(pc1, w1, equal_nan=True) and np.array_equal(pc2, w2, equal_nan=True)
    assert np.array_equal(dmean, wmean, equal_nan=True)
    if k >= 256:
        assert 0.3 * k < flipped < 0.7 * k and (wn == 0).all(1).any() and np.isnan(wn).any()
    # without the principal directions and the mean: the same normals, nothing else written
    n2, none1, none2 = hip_ops.render_orient(_cuda(rays), frame_v=_cuda(V))
    assert none1 is None and none2 is None and np.array_equal(n2.cpu().numpy(), wn, equal_nan=True)


@pytest.mark.parametrize("k", ROWS)
def test_orient_gradients(k):
    rng = _rng("grad", k)
    g = (rng.standard_normal((k, 3)) * 10.0 ** rng.uniform(-3, 3, (k, 1))).astype(np.float32)
    g[0] = [3, 0, -4]
    assert (g != 0).any(1).all()
    want = RO.orient_grad(g)
    n, none1, none2 = hip_ops.render_orient(None, grad=_cuda(g))
    n = n.cpu().numpy()
    print(f"gradient normals k = {k}: max |n - oracle| {np.abs(n - want).max():.3e}")
    assert none1 is None and none2 is None and n.dtype == np.float64 and np.array_equal(n, want)


# ---- percentile bounds -----------------------------------------------------------------------------------------------------------
QS = [(5, 95), (0, 100), (1, 99), (2.5, 97.5), (50, 50)]


def percentile_inputs(k):
    """name -> (k,) float32.  `+ 0.0` turns every -0.0 into 0.0: the two compare equal, so where a sort or a partition leaves
    which of them is not defined, in numpy or anywhere else."""
    rng = _rng("percentile", k)
    base = rng.standard_normal(k)
    out = {f"scale {s:g}": (base * s).astype(np.float32) + np.float32(0) for s in (1e-3, 1.0, 37.5, 1e3)}
    out["shifted"] = (base * 0.01 + 40.0).astype(np.float32)
    out["ties"] = np.round(base * 3, 1).astype(np.float32) + np.float32(0)
    out["all equal"] = np.full(k, np.float32(-2.7182817))
    return out


@pytest.mark.parametrize("k", [1, 2, 3, 255, 256, 257, 3130, 100003])
def test_percentile_bounds(k):
    """Bit-equal to np.percentile on the float32 column."""
    wrong, total = [], 0
    for name, c in percentile_inputs(k).items():
        dc = _cuda(c)
        for ql, qh in QS:
            got = hip_ops.render_percentile_bounds(dc, ql, qh)
            assert got.dtype == torch.float32 and got.device.type == "cuda" and tuple(got.shape) == (2,)
            got, want = got.cpu().numpy(), RO.percentile_bounds(c, ql, qh)
            total += 1
            if got.tobytes() != want.tobytes():
                wrong.append((name, ql, qh, got.tolist(), want.tolist()))
    print(f"percentile bounds k = {k}: {len(wrong)} of {total} pairs differ from np.percentile" + "".join(
        f"\n  {n} q = ({a}, {b}): {g} for {w_}" for n, a, b, g, w_ in wrong[:6]))
    assert not wrong


# ---- colour map ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lut():
    lut = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g15_render.npz"))["lut"]
    lut.setflags(write=False)
    return lut


def colormap_inputs(k, lo, hi):
    """Random float32 values from below lo to above hi; planted from the front: lo, hi, the float32 next to each on either side,
    NaN, and lo + j (hi - lo) / 256 for j at both ends and in the middle of the table."""
    rng = _rng("colormap", k, float(lo))
    c = rng.uniform(lo - 0.2 * (hi - lo + 1), hi + 0.2 * (hi - lo + 1), k).astype(np.float32)
    step = np.float32(hi - lo) / np.float32(256)
    planted = [lo, hi, np.nan, np.nextafter(lo, np.float32(-np.inf)), np.nextafter(lo, np.float32(np.inf)),
               np.nextafter(hi, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))]
    planted += [lo + np.float32(j) * step for j in (1, 2, 3, 64, 127, 128, 129, 200, 254, 255, 256)]
    planted = np.array(planted, dtype=np.float32)[:k]
    c[:len(planted)] = planted
    return c


@pytest.mark.parametrize("k", ROWS)
def test_colormap(k):
    lut = _lut()
    dlut = _cuda(lut)
    for lo, hi in ((np.float32(-5.9151087), np.float32(7.15263)), (np.float32(0.25), np.float32(0.75)), (np.float32(1.5), np.float32(1.5))):
        c = colormap_inputs(k, lo, hi)
        bounds = np.array([lo, hi], np.float32)
        want = RO.colormap(c, bounds, lut)
        got = hip_ops.render_colormap(_cuda(c), _cuda(bounds), dlut).cpu().numpy()
        rows = RO.colormap_rows(c, bounds)
        print(f"colour map k = {k}, bounds ({lo}, {hi}): {len(np.unique(rows))} distinct rows, {int((rows < 0).sum())} without one, "
              f"{int((got != want).any(1).sum())} colours differ")
        assert got.shape == (k, 3) and got.dtype == np.float64
        assert np.array_equal(got, want)
        if hi == lo:
            assert not got.any()
        elif k >= 255:
            assert {-1, 0, 1, 2, 3, 64, 127, 128, 129, 200, 254, 255} <= set(rows.tolist())


# ---- shading and the 8-bit finish ------------------------------------------------------------------------------------------------
LIGHT, EYE = [0.0, 0.0, 10.0], [0.0, 3.0, 0.5]
SYN_N = np.array([[0, 1, 0], [0, -1, 0], [1, 0, 0], [0, 0.6, -0.8], [0, -0.6, 0.8], [0, 0.6, 0.8]], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def _scene(k, m):
    """k hits among m rays: positions in the box, unit normals of which a third is scaled off unit length (about half of all face
    away from the light), principal directions orthogonal to the normal, table colours.  Planted from the front as far as k allows:
    six hits at (0, 0, 0.5) — straight under the light — whose Ward weight is +inf, -inf and NaN."""
    rng = _rng("scene", k, m)
    hits = np.zeros(m, bool); hits[rng.permutation(m)[:k]] = True
    samples = rng.uniform(-1, 1, (m, 3))
    n = rng.standard_normal((k, 3)); n /= np.linalg.norm(n, axis=1)[:, None]
    t = rng.standard_normal((k, 3))
    pc1 = np.cross(n, t); pc1 /= np.linalg.norm(pc1, axis=1)[:, None]
    pc2 = np.cross(n, pc1)
    n[::3] *= rng.uniform(0.5, 1.7, (len(n[::3]), 1))
    p = min(k, 6)
    n[:p] = SYN_N[:p]; pc1[:p] = [1, 0, 0]; pc2[:p] = np.cross(SYN_N[:p], pc1[:p])
    samples[np.flatnonzero(hits)[:p]] = [0, 0, 0.5]
    cmap = _lut()[rng.randint(0, 256, k)]
    for a in (hits, samples, n, pc1, pc2, cmap):
        a.setflags(write=False)
    return hits, samples, n, pc1, pc2, cmap


def _device_shade(model, scene, acc, with_cmap=True, **kw):
    hits, samples, n, pc1, pc2, cmap = scene
    rows = np.flatnonzero(hits).astype(np.int32)
    extra = dict(pc1=_cuda(pc1), pc2=_cuda(pc2), camera_position=EYE) if model == "ward" else {}
    hip_ops.render_shade(model, _cuda(hits.astype(np.uint8)), _cuda(rows), _cuda(samples[hits]), _cuda(n), acc, LIGHT,
                         color_map=_cuda(cmap) if with_cmap else None, **extra, **kw)


@pytest.mark.parametrize("k", SMALL)
def test_shade(k):
    """Two calls into one accumulator per model; every pixel within 1e-9 of the sum of the oracle's two images (the bound of
    test_render_gpu.py's shading tests)."""
    m = k + 1 + k // 3
    scene = _scene(k, m)
    hits, samples, n, pc1, pc2, cmap = scene
    away = int((RO._light(LIGHT, samples[hits], n)[1] <= 0).sum())
    worst = 0.0
    for sh in (-1, 0, 20):
        acc = torch.zeros(m, 3, dtype=torch.float64, device=DEV)
        _device_shade("blinn-phong", scene, acc, shininess=sh)
        _device_shade("blinn-phong", scene, acc, with_cmap=False, shininess=sh)
        want = RO.phong(LIGHT, sh, hits, samples, n, color_map=cmap) + RO.phong(LIGHT, sh, hits, samples, n)
        d = np.abs(acc.cpu().numpy() - want).max()
        print(f"phong k = {k} of m = {m}, shininess {sh}: max |acc - oracle| {d:.3e} ({away} hits face away from the light)")
        worst = max(worst, d)
        assert np.all(want[~hits] == 2.0)
    with np.errstate(all="ignore"):
        wgt = 1 / np.sqrt(RO._light(LIGHT, samples[hits], n)[1] * RO._dot(n, RO.normalize(np.array(EYE)[None] - samples[hits])))
    for a1, a2 in ((0.2, 0.2), (0.15, 0.4)):
        acc = torch.zeros(m, 3, dtype=torch.float64, device=DEV)
        _device_shade("ward", scene, acc, alpha1=a1, alpha2=a2)
        _device_shade("ward", scene, acc, with_cmap=False, alpha1=a1, alpha2=a2)
        want = RO.ward(LIGHT, EYE, hits, samples, n, a1, a2, pc1, pc2, color_map=cmap) + RO.ward(LIGHT, EYE, hits, samples, n, a1, a2, pc1, pc2)
        d = np.abs(acc.cpu().numpy() - want).max()
        print(f"ward k = {k} of m = {m}, alphas ({a1}, {a2}): max |acc - oracle| {d:.3e}; weights: {int(np.isnan(wgt).sum())} NaN, "
              f"{int(np.isposinf(wgt).sum())} +inf, {int(np.isneginf(wgt).sum())} -inf")
        worst = max(worst, d)
    assert np.isposinf(wgt).any()
    if k >= 255:
        assert np.isneginf(wgt).any() and np.isnan(wgt).any() and 0.25 * k < away < 0.75 * k
    assert worst <= 1e-9


@pytest.mark.parametrize("model", ["blinn-phong", "ward"])
def test_shade_large(model):
    """The second trip of the shading and background loops: more than 4096 * 256 hits among more rays still."""
    m = BIG + 4097
    scene = _scene(BIG, m)
    hits, samples, n, pc1, pc2, cmap = scene
    acc = torch.zeros(m, 3, dtype=torch.float64, device=DEV)
    if model == "ward":
        _device_shade("ward", scene, acc, alpha1=0.15, alpha2=0.4)
        want = RO.ward(LIGHT, EYE, hits, samples, n, 0.15, 0.4, pc1, pc2, color_map=cmap)
    else:
        _device_shade("blinn-phong", scene, acc, shininess=20)
        want = RO.phong(LIGHT, 20, hits, samples, n, color_map=cmap)
    got = acc.cpu().numpy()
    d = np.abs(got - want)
    print(f"{model} k = {BIG} of m = {m}: max |acc - oracle| {d.max():.3e}, in the last 300 hits {d[np.flatnonzero(hits)[-300:]].max():.3e}")
    assert np.all(got[~hits] == 1.0) and d.max() <= 1e-9


@pytest.mark.parametrize("count", ROWS)
@pytest.mark.parametrize("rate", [1, 2])
def test_finish(count, rate):
    """uint8 equal to the oracle's on values in [0, rate]: j / 255 * rate for every j (both sides of every truncation), 0.9 * rate
    (the shading's ceiling), rate itself (background), random ones.  No NaN: numpy's own cast of NaN to uint8 is platform-defined,
    so the oracle has no say there."""
    rng = _rng("finish", count, rate)
    acc = rng.uniform(0, rate, count)
    j = np.arange(256)
    planted = np.concatenate([[rate, 0.9 * rate, 0.0], j / 255 * rate, np.nextafter(j / 255 * rate, -1.0).clip(0), np.nextafter(j / 255 * rate, 9.0).clip(0, rate)])
    planted = planted[:count]
    acc[:len(planted)] = planted
    acc[-1] = rate
    want = RO.finish(acc, rate)
    got = hip_ops.render_finish(_cuda(acc), rate).cpu().numpy()
    print(f"finish count = {count}, sample_rate {rate}: {int((got != want).sum())} bytes differ, {len(np.unique(want))} distinct values")
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)
    if count >= 255:
        assert want[0] == 255 and want[1] == 229 and want[-1] == 255
    acc3 = acc[:count - count % 3].reshape(-1, 3) if count >= 3 else None             # the (m,3) accumulator keeps its shape
    if acc3 is not None:
        assert np.array_equal(hip_ops.render_finish(_cuda(acc3), rate).cpu().numpy(), RO.finish(acc3, rate))
