# coding: utf-8
"""GPU: sphere-traced images against tests/golden/g15_render.npz (the reference's own run, tests/golden/make_golden_st.py), stage by
stage — every stage is fed the FIXTURE's inputs, so that stages do not compound — then one pass and the whole script end to end.
Square images only (the reference swaps width and height between get_pixels_camera and its reshape).  Each test prints the figures
it measures before it asserts."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HID = [128] * 4
CAMERAS = {"obl": [0.8939, 0.7, 2.86], "pz": [0, 0, 2.9], "nz": [0, 0, -2.9]}
SCENE_CAMERA = {"a": "obl", "b": "obl", "c": "pz", "d": "obl"}


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(HERE, "golden", "g15_render.npz"))


@pytest.fixture(scope="module")
def model():
    from diffudf_amd.model import SIREN
    theta = np.load(os.path.join(HERE, "golden", "g14_pointcloud.npz"))["t_theta"]
    m = SIREN(3, 1, HID, w0=30).cuda()
    with torch.no_grad():
        m.flat_parameters().copy_(torch.from_numpy(np.ascontiguousarray(theta)).cuda())
    return m


def _configs(G, s):
    rc = json.loads(str(G[f"{s}_config"]))
    nc = {"alpha": 100, "device": 0, "gt_mode": rc.pop("gt_mode"), "hidden_layer_nodes": HID, "w0": 30, "model_path": None}
    return nc, rc


def _full(G, s, what):
    """(M,3) image of scene s from the fixture's hit rows: 1.0 elsewhere; grey scenes are stored as one channel."""
    s0 = "a" if s == "b" else s
    hits = G[f"{s0}_hits"]
    img = np.ones((len(hits), 3))
    v = G[what]
    img[hits] = v if v.ndim == 2 else v[:, None]
    return img, hits


@pytest.mark.parametrize("cam", ["obl", "pz", "nz"])
def test_ray_setup(G, cam):
    """rays and start positions to 1e-12, mask identical, for the oblique camera and the two on the z axis (the wide one sees rays
    that miss the box: t0 = 0 there)."""
    import generate_st
    from diffudf_amd import hip_ops
    n = int(G["size"])
    fov = float(G["nz_fov"]) if cam == "nz" else 45
    rays, t0, mask = hip_ops.render_setup_rays(n, n, fov, float(G["jitter"][0]), generate_st.camera_rotation(CAMERAS[cam]), CAMERAS[cam],
                                               [1, -1, 1, -1, 1, -1], "cuda:0")
    rays, t0, mask = rays.cpu().numpy(), t0.cpu().numpy(), mask.cpu().numpy().astype(bool)
    sub = slice(None, None, 8) if cam == "nz" else slice(None)
    er, et = np.abs(rays[sub] - G[cam + "_rays"]).max(), np.abs(t0[sub] - G[cam + "_t0"]).max()
    print(f"set-up {cam}: max |rays - ref| {er:.3e}, max |t0 - ref| {et:.3e}, valid {int(mask.sum())}")
    assert np.array_equal(mask, G[cam + "_mask"])
    assert er <= 1e-12 and et <= 1e-12
    assert np.all(t0[~mask] == 0.0)


def _ward_args(G):
    hits = G["a_hits"]
    samples = np.zeros((len(hits), 3)); samples[hits] = G["a_pos"]
    return hits, samples


def test_phong_shading_on_fixture_inputs(G):
    """1e-9 absolute on every pixel, with the colour map and a specular term (scene a, shininess 20)."""
    from src.render_st import phong_shading
    hits, samples = _ward_args(G)
    _, rc = _configs(G, "a")
    got = phong_shading(rc["light_position"], rc["shininess"], hits, samples, G["a_normals"].astype(np.float64),
                        color_map=G["lut"][G["a_cmap_rows"]])
    want, _ = _full(G, "a", "a_img")
    print(f"phong + colour map: max |diff| {np.abs(got - want).max():.3e}")
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-9
    # no specular at all (the reference's configs: shininess -1) is the same call with the term switched off
    got0 = phong_shading(rc["light_position"], -1, hits, samples, G["a_normals"].astype(np.float64))
    assert np.all(got0[~hits] == 1.0) and np.all(got0[hits] <= 0.9) and np.all(got0[hits] >= 0.2 - 1e-12)


@pytest.mark.parametrize("case", ["equal", "unequal", "synthetic"])
def test_ward_reflectance_on_fixture_inputs(G, case):
    """1e-9 absolute on every pixel, rows whose Ward weight is NaN or +-inf included (np.nan_to_num's outcome)."""
    from src.render_st import ward_reflectance
    if case == "synthetic":
        a1, a2 = G["syn_alphas"]
        got = ward_reflectance(list(G["syn_light"]), list(G["syn_camera"]), np.ones(6, bool), G["syn_pos"], G["syn_normals"], a1, a2,
                               G["syn_pc1"], G["syn_pc2"], color_map=G["syn_cmap"])
        want = G["syn_img"]
    else:
        hits, samples = _ward_args(G)
        _, rc = _configs(G, "b")
        a1, a2 = (rc["alpha1"], rc["alpha2"]) if case == "equal" else G["wardx_alphas"]
        pcd = G["b_pcd"].astype(np.float64)
        got = ward_reflectance(rc["light_position"], rc["camera_position"], hits, samples, G["a_normals"].astype(np.float64), a1, a2,
                               pcd[..., 0], pcd[..., 1], color_map=G["lut"][G["b_cmap_rows"]])
        want, _ = _full(G, "b", "b_img" if case == "equal" else "wardx_img")
    print(f"ward {case}: max |diff| {np.abs(got - want).max():.3e}")
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-9


@pytest.mark.parametrize("s", ["a", "b"])
def test_orientation_and_colormap(G, s):
    """On the fixture's raw eigen-frames and float32 curvatures: oriented normals and mean curvature equal the reference's, the
    percentile bounds equal np.percentile's bit for bit, the colour-table row is identical on every hit (clip, subtract, divide and
    multiply are single float32 operations on both sides), and the colour is equal to 1e-12."""
    from diffudf_amd import hip_ops
    dev = "cuda:0"
    hits = G["a_hits"]
    k = int(hits.sum())
    V = np.zeros((k, 3, 3), np.float32)
    V[:, :, :2] = G["b_pcd"]; V[:, :, 2] = G["a_normals_raw"]
    rays = torch.from_numpy(G["obl_rays"][hits]).to(dev)
    curv = torch.from_numpy(G[f"{s}_curv_raw"].copy()).to(dev)
    normals, pc1, pc2 = hip_ops.render_orient(rays, frame_v=torch.from_numpy(V).to(dev), mean=curv if s == "a" else None, want_pc=True)
    assert np.array_equal(normals.cpu().numpy(), G["a_normals"].astype(np.float64))
    assert np.array_equal(pc1.cpu().numpy(), G["b_pcd"][..., 0].astype(np.float64)) and np.array_equal(pc2.cpu().numpy(), G["b_pcd"][..., 1].astype(np.float64))
    assert np.array_equal(curv.cpu().numpy(), G[f"{s}_curv"])                   # 'mean' is re-oriented, 'gaussian' is not
    _, rc = _configs(G, s)
    bounds = hip_ops.render_percentile_bounds(curv, rc["curv_low_bound"], rc["curv_high_bound"])
    lut = torch.from_numpy(G["lut"]).to(dev)
    col = hip_ops.render_colormap(curv, bounds, lut).cpu().numpy()
    want = G["lut"][G[f"{s}_cmap_rows"]]
    same = (col == want).all(1)
    print(f"scene {s}: bounds {bounds.cpu().numpy()} (reference {G[f'{s}_bounds']}), table row identical on {same.mean():.5f} of {k} hits")
    assert bounds.cpu().numpy().tobytes() == G[f"{s}_bounds"].tobytes()
    assert same.mean() == 1.0
    assert np.abs(col[same] - want[same]).max() <= 1e-12
    assert all((row == G["lut"]).all(1).any() for row in col[~same])            # every colour is a row of the table


def _compare(tag, got, got_hits, want, want_hits, G, s, unit=1.0):
    flips = float((got_hits != want_hits).mean())
    both = got_hits & want_hits
    diff = np.abs(got[both] - want[both]).reshape(-1) / unit
    p50, p99 = float(np.percentile(diff, 50)), float(np.percentile(diff, 99))
    fate, r50, r99 = float(G[f"{s}_fate"]), float(G[f"{s}_coldiff_p50"]), float(G[f"{s}_coldiff_p99"])
    a_f, a_50, a_99 = 2 * (1 - fate), 2 * r50 / unit, 2 * r99 / unit
    print(f"{tag}: hit/miss differs on {flips:.5f} of the pixels (allowed {a_f:.5f}); colour difference p50 {p50:.3e} "
          f"(allowed {a_50:.3e}) p99 {p99:.3e} (allowed {a_99:.3e}); max {diff.max():.3e}")
    return flips, p50, p99, a_f, a_50, a_99


@pytest.mark.parametrize("s", ["a", "b", "c", "d"])
def test_one_pass_end_to_end(G, model, s):
    """create_projectional_image on the fixture's rays, start positions and mask.  Pixels whose hit / miss differs from the
    reference's float32 run: at most 2 (1 - fate) of that scene; on pixels that hit in both, median and 99th percentile of the
    colour difference within twice the fixture's float32-against-float64 figures.  t0 and mask_rays come back updated in place."""
    from src.render_st import create_projectional_image
    nc, rc = _configs(G, s)
    cam = SCENE_CAMERA[s]
    rays, t0, mask = G[cam + "_rays"].copy(), G[cam + "_t0"].copy(), G[cam + "_mask"].copy()
    img = create_projectional_image(model, rays, t0, mask, nc, rc, torch.device("cuda:0"), colormap=G["lut"])
    n = int(G["size"])
    assert img.shape == (n, n, 3) and img.dtype == np.float64
    img = img.reshape(-1, 3)
    want, want_hits = _full(G, s, f"{s}_img")
    got_hits = ~(img == 1.0).all(1)
    flips, p50, p99, a_f, a_50, a_99 = _compare(f"one pass, scene {s}", img, got_hits, want, want_hits, G, s)
    s0 = "a" if s == "b" else s
    both = (got_hits & want_hits)[want_hits]
    print(f"  positions of common hits: max |t0 - ref| {np.abs(t0[want_hits][both] - G[f'{s0}_pos'][both]).max():.3e}; "
          f"mask_rays equal on {(mask == G[f'{s0}_mask_after']).mean():.5f} of the rays")
    assert not np.array_equal(t0, G[cam + "_t0"]) and mask.sum() < G[cam + "_mask"].sum()         # updated in place
    assert flips <= a_f
    assert p50 <= a_50 and p99 <= a_99


def test_whole_script(G, model, tmp_path):
    """render(config, jitter = the fixture's) against the reference's final uint8 image of scene a (both passes), the same two
    criteria in units of 1/255; a second call is bit-identical; generate_st with a seeded np.random draws the fixture's jitter."""
    import generate_st
    nc, rc = _configs(G, "a")
    ckpt = str(tmp_path / "model.pth")
    torch.save(model.state_dict(), ckpt)
    nc["model_path"] = ckpt
    cfg = {"network_config": nc, "rendering_config": rc}
    img = generate_st.render(cfg, jitter=G["jitter"], colormap=G["lut"])
    n = int(G["size"])
    assert img.shape == (n, n, 3) and img.dtype == np.uint8
    again = generate_st.render(cfg, jitter=G["jitter"], colormap=G["lut"])
    assert np.array_equal(img, again)
    want = G["a_final"].reshape(-1, 3).astype(np.float64)
    got = img.reshape(-1, 3).astype(np.float64)
    flips, p50, p99, a_f, a_50, a_99 = _compare("whole script, scene a (units of 1/255)", got / 255, (got != 255).any(1), want / 255,
                                                (want != 255).any(1), G, "a", unit=1 / 255)
    assert flips <= a_f
    assert p50 <= a_50 and p99 <= a_99
    # the script itself: same jitter from the same seed, a PIL image (or the array without PIL) of the same content
    np.random.seed(int(G["seed"]))
    im = generate_st.generate_st(cfg)
    assert np.array_equal(np.asarray(im), img)
    np.random.seed(int(G["seed"]))
    assert np.allclose([np.random.normal(0.5, 0.35) for _ in range(2)], G["jitter"], rtol=0, atol=0)


def test_errors_and_sample_rates(G, model):
    import generate_st
    from diffudf_amd._lib import DudfError
    from diffudf_amd.model import SIREN
    from src.render_st import create_projectional_image
    nc, rc = _configs(G, "c")
    cfg = {"network_config": nc, "rendering_config": dict(rc, width=32, height=32)}
    for rate in (1, 3):
        cfg["rendering_config"]["sample_rate"] = rate
        img = generate_st.render(cfg, jitter=[0.5] * rate, model=model)
        assert img.shape == (32, 32, 3) and img.dtype == np.uint8 and (img != 255).any() and (img == 255).any()
    # a camera inside the box looking at an empty corner region never converges: the reference's ValueError
    blind = dict(rc, width=16, height=16, surface_threshold=1e-30, max_iterations=2)
    with pytest.raises(ValueError, match="did not converge"):
        generate_st.render({"network_config": nc, "rendering_config": blind}, jitter=[0.5, 0.5], model=model)
    # CPU model / missing colour table
    cpu_model = SIREN(3, 1, HID, w0=30)
    rays, t0, mask = G["pz_rays"].copy(), G["pz_t0"].copy(), G["pz_mask"].copy()
    with pytest.raises(DudfError):
        create_projectional_image(cpu_model, rays, t0, mask, nc, rc, torch.device("cpu"))
    nca, rca = _configs(G, "a")
    with pytest.raises(DudfError, match="256,3"):
        create_projectional_image(model, rays, t0, mask, nca, rca, torch.device("cuda:0"), colormap=np.zeros((10, 3)))
    from diffudf_amd import hip_ops
    acc = torch.zeros(len(mask), 3, dtype=torch.float64, device="cuda:0")
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()            # noqa: E731
    with pytest.raises(DudfError, match="colour table"):
        hip_ops.render_traced(model.hip_cfg, model.flat_parameters(), d(rays), d(t0), d(mask.astype(np.uint8)), nca, rca, None, acc)
