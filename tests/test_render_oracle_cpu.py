# coding: utf-8
"""CPU: tests/render_oracle.py against the reference's own run (tests/golden/g15_render.npz) — every stage of the oracle is fed the
fixture's inputs and must give the fixture's outputs, before tests/test_render_stages_gpu.py lets it judge the kernels."""
import json
import os

import numpy as np
import pytest

import render_oracle as RO

HERE = os.path.dirname(os.path.abspath(__file__))
CAMERAS = {"obl": [0.8939, 0.7, 2.86], "pz": [0, 0, 2.9], "nz": [0, 0, -2.9]}


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(HERE, "golden", "g15_render.npz"))


def _config(G, s):
    return json.loads(str(G[f"{s}_config"]))


def _frames(G):
    k = int(G["a_hits"].sum())
    V = np.zeros((k, 3, 3), np.float32)
    V[:, :, :2] = G["b_pcd"]; V[:, :, 2] = G["a_normals_raw"]
    return V


def _image(G, what):
    img = np.ones((len(G["a_hits"]), 3))
    img[G["a_hits"]] = G[what]
    return img


def _samples(G):
    samples = np.zeros((len(G["a_hits"]), 3)); samples[G["a_hits"]] = G["a_pos"]
    return samples


@pytest.mark.parametrize("cam", ["obl", "pz", "nz"])
def test_setup_rays(G, cam):
    import generate_st
    n = int(G["size"])
    fov = float(G["nz_fov"]) if cam == "nz" else 45
    rays, t0, mask, margin = RO.setup_rays(n, n, fov, float(G["jitter"][0]), generate_st.camera_rotation(CAMERAS[cam]), CAMERAS[cam])
    sub = slice(None, None, 8) if cam == "nz" else slice(None)
    er, et = np.abs(rays[sub] - G[cam + "_rays"]).max(), np.abs(t0[sub] - G[cam + "_t0"]).max()
    print(f"oracle set-up {cam}: max |rays - ref| {er:.3e}, max |t0 - ref| {et:.3e}, smallest decision margin {margin.min():.3e}")
    assert np.array_equal(mask, G[cam + "_mask"])
    assert er <= 1e-12 and et <= 1e-12
    assert rays.dtype == t0.dtype == np.float64 and np.all(t0[~mask] == 0.0)
    assert margin.shape == mask.shape and np.all(margin >= 0)


def test_orientation_bit_for_bit(G):
    hits = G["a_hits"]
    V = _frames(G)
    normals, pc1, pc2, mean = RO.orient_frame(V, G["obl_rays"][hits], G["a_curv_raw"])
    assert normals.dtype == np.float64 and mean.dtype == np.float32
    assert np.array_equal(normals, G["a_normals"].astype(np.float64))
    assert np.array_equal(pc1, G["b_pcd"][..., 0].astype(np.float64)) and np.array_equal(pc2, G["b_pcd"][..., 1].astype(np.float64))
    assert np.array_equal(mean, G["a_curv"])
    assert (normals != G["a_normals_raw"]).any()                                   # the fixture does turn some normals
    assert np.array_equal(G["b_curv"], G["b_curv_raw"])                            # 'gaussian' is not re-oriented
    assert RO.orient_frame(V, G["obl_rays"][hits])[3] is None
    # planted: n . ray == 0 gives align = -0.0, NaN gives NaN (np.sign)
    e = np.zeros((2, 3, 3), np.float32); e[:, :, 2] = [0, 0, 1]; e[1, 0, 2] = np.nan
    n, _, _, m = RO.orient_frame(e, np.array([[1.0, 0, 0], [1.0, 0, 0]]), np.float32([2, 2]))
    assert np.array_equal(n[0], [0, 0, 0]) and np.signbit(n[0, 2]) and m[0] == 0 and np.isnan(n[1]).all() and np.isnan(m[1])


def test_orient_grad():
    g = np.float32([[3, 0, 4], [0, 0, 0], [1e-3, -2e-3, 2e-3]])
    n = RO.orient_grad(g)
    assert n.dtype == np.float64 and np.array_equal(n[0], np.float32([0.6, 0, 0.8]).astype(np.float64)) and np.isnan(n[1]).all()
    assert np.array_equal(n, n.astype(np.float32).astype(np.float64), equal_nan=True) and abs(np.linalg.norm(n[2]) - 1) < 1e-6


@pytest.mark.parametrize("s", ["a", "b"])
def test_percentile_bounds_bit_for_bit(G, s):
    rc = _config(G, s)
    got = RO.percentile_bounds(G[f"{s}_curv"], rc["curv_low_bound"], rc["curv_high_bound"])
    want = G[f"{s}_bounds"]
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), (
        f"np.percentile of numpy {np.__version__} gives {got!r} on the fixture's float32 curvatures, the fixture holds {want!r}: "
        "the installed numpy is not the one tests/golden/g15_render.npz speaks for (it interpolates float32 percentiles in "
        "float32: numpy 2.x), so this oracle cannot judge hip_ops.render_percentile_bounds here")


@pytest.mark.parametrize("s", ["a", "b"])
def test_colormap_rows_on_every_hit(G, s):
    rows = RO.colormap_rows(G[f"{s}_curv"], G[f"{s}_bounds"])
    same = rows == G[f"{s}_cmap_rows"]
    print(f"scene {s}: table row identical on {same.mean():.5f} of {len(rows)} hits")
    assert same.all()
    assert np.array_equal(RO.colormap(G[f"{s}_curv"], G[f"{s}_bounds"], G["lut"]), G["lut"][G[f"{s}_cmap_rows"]])


def test_colormap_edges(G):
    lut = G["lut"]
    b = np.float32([-1, 3])
    step = np.float32(4) / np.float32(256)
    c = np.float32([-1, 3, -2, 4, np.nan, -1 + 7 * step, 3 - step])
    assert RO.colormap_rows(c, b).tolist() == [0, 255, 0, 255, -1, 7, 255]
    col = RO.colormap(c, b, lut)
    assert np.array_equal(col[4], [0, 0, 0]) and np.array_equal(col[1], lut[255]) and np.array_equal(col[5], lut[7])
    assert (RO.colormap_rows(c, np.float32([2, 2])) == -1).all() and not RO.colormap(c, np.float32([2, 2]), lut).any()


def test_colormap_is_matplotlibs(G):
    try:
        import matplotlib
    except ImportError:
        return                                                                     # the table itself is pinned in test_render_cpu.py
    cmap = matplotlib.colormaps['RdYlBu']
    for s in "ab":
        c = G[f"{s}_curv"].copy()
        lo, hi = G[f"{s}_bounds"]
        c = np.clip(c, lo, hi); c -= np.min(c); c /= np.max(c)
        assert np.array_equal(RO.colormap(G[f"{s}_curv"], G[f"{s}_bounds"], G["lut"]), cmap(c)[:, :3])
    c = np.float32([0.0, 0.25, np.nan, 1.0, 0.999])                                # bounds (0, 1): the values are matplotlib's input
    assert np.array_equal(RO.colormap(c, np.float32([0, 1]), G["lut"]), cmap(c)[:, :3])


def test_phong_images(G):
    rc = _config(G, "a")
    got = RO.phong(rc["light_position"], rc["shininess"], G["a_hits"], _samples(G), G["a_normals"].astype(np.float64),
                   color_map=G["lut"][G["a_cmap_rows"]])
    d = np.abs(got - _image(G, "a_img")).max()
    print(f"oracle phong + colour map: max |diff| {d:.3e}")
    assert d <= 1e-9
    grey = RO.phong(rc["light_position"], -1, G["a_hits"], _samples(G), G["a_normals"].astype(np.float64))
    assert np.all(grey[~G["a_hits"]] == 1.0) and np.all(grey[G["a_hits"]] <= 0.9) and np.all(grey[G["a_hits"]] >= 0.2 - 1e-12)


@pytest.mark.parametrize("case", ["equal", "unequal", "synthetic"])
def test_ward_images(G, case):
    if case == "synthetic":
        a1, a2 = G["syn_alphas"]
        got = RO.ward(list(G["syn_light"]), list(G["syn_camera"]), np.ones(6, bool), G["syn_pos"], G["syn_normals"], a1, a2,
                      G["syn_pc1"], G["syn_pc2"], color_map=G["syn_cmap"])
        want = G["syn_img"]
    else:
        rc = _config(G, "b")
        a1, a2 = (rc["alpha1"], rc["alpha2"]) if case == "equal" else G["wardx_alphas"]
        pcd = G["b_pcd"].astype(np.float64)
        got = RO.ward(rc["light_position"], rc["camera_position"], G["a_hits"], _samples(G), G["a_normals"].astype(np.float64), a1, a2,
                      pcd[..., 0], pcd[..., 1], color_map=G["lut"][G["b_cmap_rows"]])
        want = _image(G, "b_img" if case == "equal" else "wardx_img")
    d = np.abs(got - want).max()
    print(f"oracle ward {case}: max |diff| {d:.3e}")
    assert got.shape == want.shape and d <= 1e-9


def test_gather_and_finish(G):
    hits = G["a_hits"]
    pos, rays, rows, k = RO.gather(hits, G["obl_t0"], G["obl_rays"])
    assert k == int(hits.sum()) == len(pos) and rows.dtype == np.int32 and np.array_equal(rows, np.nonzero(hits)[0])
    assert np.array_equal(pos, G["obl_t0"][rows]) and np.array_equal(rays, G["obl_rays"][rows])
    # the fixture holds the image of ONE pass of scene a next to the final image of two, so `finish` has no accumulator of the
    # fixture's to run on: constructed values only.  j / 255 * rate comes back as j or, where the quotient rounds down, j - 1.
    for rate in (1, 2):
        j = np.arange(256)
        out = RO.finish(j / 255 * rate, rate)
        assert out.dtype == np.uint8 and np.all((out == j) | (out == j - 1)) and (out == j).mean() > 0.9
        assert RO.finish(np.array([0.0, 0.9 * rate, rate]), rate).tolist() == [0, 229, 255]
    assert np.array_equal(RO.finish(np.full((2, 3), 2.0), 2), np.full((2, 3), 255, np.uint8))
