# coding: utf-8
"""Plain numpy restatement of the image stages of generate_st around the marching loop (csrc/dudf_render.hip and
`hip_ops.render_percentile_bounds`), for tests/test_render_oracle_cpu.py — which pins every function here to the reference's own
run (tests/golden/g15_render.npz) — and tests/test_render_stages_gpu.py, which holds the kernels against it at edge sizes.

Written from reference generate_st.py:9-33, :41-101, :139, src/render_st.py:80-83, :101-114, :174-245 and src/util.py:34-39, in
that order of operations and with those dtypes: float32 where torch hands float32 over (eigen-frames, gradients, curvatures),
float64 wherever a float64 operand promotes.  Sums of three are numpy's: (a0 + a1) + a2.  Everything is vectorised over the rows."""
import numpy as np

import generate_st

BOX = 1.001                 # the reference accepts plane intersections up to this far out
PARALLEL = 1e-5             # |ray component| below which a plane counts as parallel to the ray


def _rownorm(a):
    """||row|| as np.linalg.norm(a, axis=1) forms it: sqrt of the summed squares, in a's dtype."""
    return np.sqrt(np.add.reduce(a * a, axis=1))


def normalize(a):
    """src/util.py:34-39 for an (n,3) array."""
    return a / _rownorm(a)[:, None]


def _dot(a, b):
    return np.sum(a * b, axis=-1)


# ---- ray set-up ------------------------------------------------------------------------------------------------------------------
def setup_rays(width, height, fov, noise, R, cam, planes=(1, -1, 1, -1, 1, -1)):
    """(rays (m,3), t0 (m,3) float64, mask (m,) bool, margin (m,) float64) of the width * height pixels, p = iy * width + ix.
    margin: the smallest distance from its threshold of any comparison that decided the ray's mask or its plane — an in-box
    coordinate against +-1.001 (planes that are not parallel only), |component| against 1e-5, an accepted plane's distance against
    0, and the gap between the two nearest accepted planes in front of the camera.  A device result may differ from this one on
    a ray whose margin is at rounding level, and nowhere else."""
    R = np.asarray(R, dtype=np.float64)
    cam64 = np.array([float(v) for v in cam])
    cam32 = np.float32(cam64)                                            # the position is added to the pixels as float32 ...
    px = generate_st.get_pixels_camera(width, height, fov, noise).reshape(width * height, 3)
    d = (R @ px.T).T + cam32
    d = d / _rownorm(d)[:, None]
    d = d * -1
    axis = np.array([0, 0, 1, 1, 2, 2])
    num = np.array([float(v) for v in planes]) - cam64[axis]             # ... and as float64 everywhere else
    den = d[:, axis]                                                     # (m,6)
    par = np.abs(den) < PARALLEL
    ds = num[None, :] / np.where(par, 1.0, den)
    q = d[:, None, :] * ds[:, :, None] + cam64[None, None, :]            # (m,6,3)
    crossing = np.abs(den) > PARALLEL
    ok = np.all((q >= -BOX) & (q <= BOX), axis=-1) & crossing
    mask = ok.any(axis=1)
    front = ok & (ds >= 0)
    cand = np.where(front, ds, np.inf)
    dmin = cand.min(axis=1)
    t0 = np.zeros_like(d)
    with np.errstate(invalid="ignore"):
        t0[mask] = d[mask] * dmin[mask, None] + cam64[None, :]
    # decision margins
    mq = np.minimum(np.abs(q - BOX), np.abs(q + BOX)).min(axis=-1)
    mq = np.where(crossing, mq, np.inf).min(axis=1)
    mden = np.abs(np.abs(den) - PARALLEL).min(axis=1)
    mfront = np.where(ok, np.abs(ds), np.inf).min(axis=1)
    two = np.sort(cand, axis=1)[:, :2]
    with np.errstate(invalid="ignore"):
        gap = np.where(np.isfinite(two[:, 1]), two[:, 1] - two[:, 0], np.inf)
    margin = np.minimum(np.minimum(mq, mden), np.minimum(mfront, gap))
    return d, t0, mask, margin


# ---- gather ----------------------------------------------------------------------------------------------------------------------
def gather(hits, t0, rays):
    """(t0[hits], rays[hits], image row of every gathered hit as int32, k)."""
    hits = np.asarray(hits).astype(bool)
    rows = np.flatnonzero(hits).astype(np.int32)
    return t0[hits], rays[hits], rows, len(rows)


# ---- normals ---------------------------------------------------------------------------------------------------------------------
def orient_frame(V32, rays, mean32=None):
    """From (k,3,3) float32 eigen-frames (columns v0, v1, v2) and the (k,3) float64 rays of the hits: the normal v2 turned against
    its ray, align = -sign(v2 . ray) with np.sign's 0 for 0 and NaN for NaN, applied to the float32 values; the principal
    directions as they are; `mean32` (k,) float32 times the same alignment.  Returns (normals, pc1, pc2 (k,3) float64, mean float32
    or None)."""
    V32 = np.asarray(V32, dtype=np.float32)
    n32 = V32[:, :, 2].copy()
    with np.errstate(invalid="ignore"):
        align = np.sign(np.sum(n32 * rays, axis=1))[:, None] * -1        # float64
        n32 *= align.astype(np.float32)                                  # in place in float32; +-1, +-0 and NaN are exact in it
        mean = None
        if mean32 is not None:
            mean = np.asarray(mean32, dtype=np.float32).reshape(-1, 1).copy()
            mean *= align.astype(np.float32)
            mean = mean[:, 0]
    return n32.astype(np.float64), V32[:, :, 0].astype(np.float64), V32[:, :, 1].astype(np.float64), mean


def orient_grad(g32):
    """'siren': the normalised float32 gradient, no orientation.  (k,3) float64 holding float32 values."""
    g32 = np.asarray(g32, dtype=np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        return normalize(g32).astype(np.float64)


# ---- curvature colours -----------------------------------------------------------------------------------------------------------
def percentile_bounds(c32, q_low, q_high):
    """The two clip bounds of src/render_st.py:111: np.percentile ITSELF on the (k,1) float32 column with the config's python
    numbers — whatever arithmetic the installed numpy uses for a float32 array is the definition."""
    col = np.asarray(c32, dtype=np.float32).reshape(-1, 1)
    return np.array([np.percentile(col, q_low), np.percentile(col, q_high)], dtype=np.float32)


def colormap_rows(c32, bounds32):
    """Row of the 256-entry colour table for every curvature, -1 for "no row" (NaN: matplotlib's bad colour).  Clip to the bounds,
    subtract the smallest value left (lo), divide by the largest left (hi - lo), times 256 as matplotlib does it — each a single
    float32 operation —, truncate, clamp to [0, 255]."""
    c = np.asarray(c32, dtype=np.float32).reshape(-1)
    lo, hi = np.float32(bounds32[0]), np.float32(bounds32[1])
    with np.errstate(invalid="ignore", divide="ignore"):
        c = np.where(c < lo, lo, np.where(c > hi, hi, c))                # np.clip: NaN stays
        x = ((c - lo) / np.float32(hi - lo)) * np.float32(256)
    assert x.dtype == np.float32
    bad = np.isnan(x)
    rows = np.clip(np.trunc(np.where(bad, 0, x)), 0, 255).astype(np.int64)
    return np.where(bad, -1, rows)


def colormap(c32, bounds32, lut):
    """(k,3) float64 colours: the table row, (0, 0, 0) where there is none."""
    rows = colormap_rows(c32, bounds32)
    out = np.asarray(lut, dtype=np.float64)[np.maximum(rows, 0)]
    out[rows < 0] = 0.0
    return out


# ---- reflection models -----------------------------------------------------------------------------------------------------------
def _paint(hits, samples, lambertian, specular, color_map):
    k = len(lambertian)
    if color_map is None:
        diffuse = np.full((k, 3), 0.7); spec_c = np.full((k, 3), 0.7); ambient = np.full((k, 3), 0.2)
    else:
        diffuse = color_map * 0.7; spec_c = color_map * 0.7; ambient = color_map * 0.2
    image = np.ones_like(samples)                                        # pixels without a hit stay 1
    with np.errstate(invalid="ignore", over="ignore"):
        image[hits] = np.clip(diffuse * lambertian[:, None] + spec_c * specular[:, None] + ambient, 0, 0.9)
    return image


def _light(light_position, x, normals):
    L = normalize(np.asarray(light_position, dtype=np.float64)[None, :] - x)
    ndl = _dot(normals, L)
    return L, ndl, np.where(np.isnan(ndl), ndl, np.maximum(ndl, 0.0))    # np.max([., 0]): NaN stays NaN


def phong(light_position, shininess, hits, samples, normals, color_map=None):
    """(M,3) float64 Blinn-Phong image of src/render_st.py:174-204: `samples` (M,3) positions of every ray, `normals` (k,3) of the
    hits in row order.  The specular term is there only for shininess > 0, and only where the light reaches the surface."""
    hits = np.asarray(hits).astype(bool)
    x = samples[hits]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        L, _, lambertian = _light(light_position, x, normals)
        I = -1 * L
        Rf = I - (2 * _dot(normals, I))[:, None] * normals
        rv = _dot(Rf, normalize(x))
        ang = np.where(np.isnan(rv), rv, np.maximum(rv, 0.0))
        specular = np.zeros_like(lambertian)
        if shininess > 0:
            lit = lambertian > 0
            specular[lit] = np.power(ang, shininess)[lit]
    return _paint(hits, samples, lambertian, specular, color_map)


def ward(light_position, camera_position, hits, samples, normals, alpha1, alpha2, pc1, pc2, color_map=None):
    """(M,3) float64 Ward image of src/render_st.py:206-245: anisotropic lobe along the principal directions, NaN weights to 0 and
    infinite ones to +-DBL_MAX (np.nan_to_num) before the factor 0.1 and the clip."""
    hits = np.asarray(hits).astype(bool)
    x = samples[hits]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        L, ndl, lambertian = _light(light_position, x, normals)
        v = normalize(np.asarray(camera_position, dtype=np.float64)[None, :] - x)
        H = normalize(v + L)
        weight = 1 / (4 * np.pi * alpha1 * alpha2 * np.sqrt(ndl * _dot(normals, v)))
        specular = weight * np.exp(-2 * ((_dot(H, pc1) / alpha1) ** 2 + (_dot(H, pc2) / alpha2) ** 2) / (1 + _dot(normals, H)))
        specular = np.nan_to_num(specular)
        specular = specular * 0.1
    return _paint(hits, samples, lambertian, specular, color_map)


# ---- 8-bit image -----------------------------------------------------------------------------------------------------------------
def finish(acc, rate):
    """generate_st.py:139.  Only for values in [0, rate]: numpy's cast of NaN or of anything outside [0, 256) is platform-defined."""
    return (np.asarray(acc, dtype=np.float64) / rate * 255).astype(np.uint8)
