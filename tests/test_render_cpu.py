# coding: utf-8
"""CPU: the host side of generate_st — pixel grid, camera rotation, PNG writer, C-ABI declarations, the fixture's own invariants
(tests/golden/g15_render.npz, made by tests/golden/make_golden_st.py from the reference itself).  Images are square throughout:
the reference swaps width and height between get_pixels_camera and its reshape."""
import os
import re
import struct
import zlib

import numpy as np
import pytest

from diffudf_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "g15_render.npz")
RENDER_SYMBOLS = ("dudf_render_setup_rays", "dudf_render_gather", "dudf_render_orient", "dudf_render_colormap", "dudf_render_shade",
                  "dudf_render_finish")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_get_pixels_camera_matches_the_reference(gold):
    import generate_st
    n = int(gold["size"])
    px = generate_st.get_pixels_camera(n, n, 45, float(gold["jitter"][0]))
    assert px.shape == (n, n, 3) and px.dtype == np.float64
    assert np.abs(px[0, :, 0] - gold["pixels_x"]).max() <= 1e-15 and np.abs(px[:, 0, 1] - gold["pixels_y"]).max() <= 1e-15
    assert np.array_equal(px[..., 0], np.tile(px[0, :, 0], (n, 1))) and np.array_equal(px[..., 1], np.tile(px[:, 0, 1][:, None], (1, n)))
    assert np.all(px[..., 2] == -1.0)


def test_camera_rotation_three_branches():
    import generate_st
    # the camera frame looks down -z: from +z it already faces the origin (a@b = 1), from -z it turns about y (a@b = -1)
    assert np.array_equal(generate_st.camera_rotation([0, 0, 2.9]), np.eye(3))
    assert np.array_equal(generate_st.camera_rotation([0, 0, -2.9]), np.diag([-1.0, 1.0, -1.0]))
    R = generate_st.camera_rotation([0.8939, 0.7, 2.86])
    b = -np.float32([0.8939, 0.7, 2.86]); b = (b / np.linalg.norm(b)).astype(np.float64)
    assert np.abs(R.T @ R - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(R) - 1) < 1e-6                # b is float32: orthonormal to that
    assert np.allclose(R[:, 2], b, atol=1e-7) and abs(R[:, 1] @ b) < 1e-7 and R[1, 1] > 0 and abs(R[1, 0]) < 1e-12
    assert np.allclose(R @ np.array([0, 0, 1.0]), b, atol=1e-7)


def test_png_writer_round_trip(tmp_path):
    import generate_st
    rng = np.random.RandomState(3)
    img = rng.randint(0, 256, size=(7, 5, 3)).astype(np.uint8)
    path = str(tmp_path / "x.png")
    generate_st.write_png(path, img)
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    o, chunks = 8, []
    while o < len(raw):
        n, tag = struct.unpack(">I", raw[o:o + 4])[0], raw[o + 4:o + 8]
        data = raw[o + 8:o + 8 + n]
        assert struct.unpack(">I", raw[o + 8 + n:o + 12 + n])[0] == zlib.crc32(tag + data) & 0xFFFFFFFF
        chunks.append((tag, data)); o += 12 + n
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    assert struct.unpack(">IIBBBBB", chunks[0][1]) == (5, 7, 8, 2, 0, 0, 0)
    rows = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(7, 1 + 5 * 3)
    assert np.all(rows[:, 0] == 0) and np.array_equal(rows[:, 1:].reshape(7, 5, 3), img)
    try:
        from PIL import Image
    except ImportError:
        return
    assert np.array_equal(np.asarray(Image.open(path)), img)
    with pytest.raises(ValueError):
        generate_st.write_png(path, np.zeros((4, 4), np.uint8))


def test_header_declares_and_library_exports_the_render_calls():
    src = open(os.path.join(REPO, "include", "dudf_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    for name in RENDER_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    # host-side argument checks run without a GPU
    assert lib.dudf_render_finish(None, -1, 1.0, None, None) == -1
    assert lib.dudf_render_shade(7, None, 0, None, 0, None, None, None, None, None, None, None, 0.0, 0.0, 0.0, None, None) == -3
    assert lib.dudf_render_setup_rays(0, 4, 45.0, 0.5, None, None, None, None, None, None, None) == -1


def test_fixture_invariants(gold):
    assert os.path.getsize(GOLD) < (1 << 20)
    for s in "abcd":
        assert float(gold[f"{s}_fate"]) >= 0.99
        assert 0 <= float(gold[f"{s}_coldiff_p50"]) <= float(gold[f"{s}_coldiff_p99"])
    n = int(gold["size"])
    assert gold["obl_rays"].shape == (n * n, 3) and gold["pz_t0"].shape == (n * n, 3) and gold["lut"].shape == (256, 3)
    assert gold["a_final"].shape == (n, n, 3) and gold["a_final"].dtype == np.uint8
    assert 0 < gold["nz_mask"].sum() < n * n                        # the set-up test sees rays that miss the box
    with np.errstate(all="ignore"):                                 # the Ward rows np.nan_to_num has to deal with are there
        nl = (gold["syn_normals"] * (gold["syn_light"] - gold["syn_pos"])).sum(1)
        nv = (gold["syn_normals"] * (gold["syn_camera"] - gold["syn_pos"])).sum(1)
        w = 1 / np.sqrt(nl * nv)
    assert np.isposinf(w).any() and np.isneginf(w).any() and np.isnan(w).any()


def test_gt_renderer_is_out_of_scope():
    from src.render_st import create_projectional_image_gt
    with pytest.raises(_lib.DudfError, match="open3d"):
        create_projectional_image_gt("mesh.obj", 4, 4, None, None, None, None, False)


def test_colormap_default_and_missing_matplotlib(monkeypatch):
    import sys
    from diffudf_amd import render_st
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        pass
    else:
        lut = render_st.default_colormap()
        assert lut.shape == (256, 3) and lut.dtype == np.float64 and np.array_equal(lut, np.load(GOLD)["lut"])
    monkeypatch.setitem(sys.modules, "matplotlib", None)            # `import matplotlib` now raises ImportError
    with pytest.raises(_lib.DudfError, match="matplotlib"):
        render_st.default_colormap()
