# coding: utf-8
"""CPU: the numpy oracle of the normal estimation and the outlier test (tests/cloudprep_oracle.py) on clouds whose answer is known, the
argument checks of the two C entry points (they return before their first HIP call: fake pointers, as in test_orient_cpu.py), and the
PLY reader on a cloud without normals."""
import ctypes
import os
import re

import numpy as np
import pytest

import cloudprep_oracle as CO
from diffudf_amd import _lib, mesh

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_CFG, E_WS, E_MODE, E_UNSUP = 0, -1, -2, -3, -4
NAMES = ("dudf_estimate_normals", "dudf_cloud_outliers")


# ---- the C entry points ------------------------------------------------------------------------------------------------------------
_arena = ctypes.create_string_buffer(1 << 20)
BASE = (ctypes.addressof(_arena) + 255) // 256 * 256
P = ctypes.c_void_p(BASE)
N = 8


def test_header_binding_and_library_agree():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "dudf_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in NAMES + tuple(n + "_workspace_bytes" for n in NAMES):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert "DUDF_ABI_VERSION 8" in src and lib.dudf_abi_version() == 8 == _lib.ABI_VERSION


def _refusals(call, size):
    nb = int(size(N, 3))
    assert 0 < nb <= (1 << 20) - 512
    assert call(N, 0, None, nb) == E_UNSUP
    assert call(N, 17, None, nb) == E_UNSUP
    assert call(1 << 31, 3, None, nb) == E_UNSUP
    assert call(-1, 3, None, nb) == E_CFG
    assert call(-1, 0, None, nb) == E_CFG                         # a negative count before K
    assert call(0, 17, None, nb) == E_UNSUP                       # K before the empty call
    assert call(0, 3, None, 0) == OK                              # n == 0: nothing is launched
    assert call(N, 3, None, nb, first=None) == E_CFG              # the inputs before the workspace
    assert call(N, 3, None, nb) == E_WS
    assert call(N, 3, ctypes.c_void_p(BASE + 8), nb) == E_WS
    assert call(N, 3, P, nb - 1) == E_WS
    assert size(N, 0) == 0 and size(N, 17) == 0 and size(-1, 3) == 0 and size(1 << 31, 3) == 0
    assert size(0, 3) > 0


def test_estimate_normals_refusals():
    lib = _lib.load()
    _refusals(lambda n, k, ws, nb, first=P: lib.dudf_estimate_normals(first, P, n, k, 1, P, P, P, ws, nb, None),
              lib.dudf_estimate_normals_workspace_bytes)
    nb = int(lib.dudf_estimate_normals_workspace_bytes(N, 3))
    assert lib.dudf_estimate_normals(P, None, N, 3, 1, P, P, P, P, nb, None) == E_CFG
    assert lib.dudf_estimate_normals(P, P, N, 3, 1, None, P, P, P, nb, None) == E_CFG
    assert lib.dudf_estimate_normals(P, P, N, 3, 1, P, None, None, None, nb, None) == E_WS      # the optional outputs may be NULL


def test_cloud_outliers_refusals():
    lib = _lib.load()
    _refusals(lambda n, k, ws, nb, first=P: lib.dudf_cloud_outliers(first, n, k, 2.0, P, P, P, P, P, ws, nb, None),
              lib.dudf_cloud_outliers_workspace_bytes)
    nb = int(lib.dudf_cloud_outliers_workspace_bytes(N, 3))
    assert lib.dudf_cloud_outliers(P, N, 3, 2.0, None, P, P, P, P, P, nb, None) == E_CFG
    assert lib.dudf_cloud_outliers(P, N, 3, 2.0, P, None, P, P, P, P, nb, None) == E_CFG
    assert lib.dudf_cloud_outliers(P, N, 3, 2.0, P, P, None, None, None, None, nb, None) == E_WS


def test_workspace_sizes_state_the_layouts():
    """Estimation: the cloud as 16-byte rows.  Outliers: 256 partial sums and counts, the statistics, two counters, then 4 + 8 bytes
    per 256-row tile — every array on its own 256-byte granule, at least one granule long."""
    lib = _lib.load()
    r = lambda b: (b + 255) // 256 * 256  # noqa: E731
    for n in (0, 1, 16, 17, 1000, 100000):
        assert lib.dudf_estimate_normals_workspace_bytes(n, 15) == r(16 * max(n, 1))
        tiles = max((n + 255) // 256, 1)
        assert lib.dudf_cloud_outliers_workspace_bytes(n, 16) == 2048 + 2048 + 3 * 256 + r(4 * tiles) + r(8 * tiles)


# ---- the oracle's own properties -----------------------------------------------------------------------------------------------------
def test_jacobi_restatement_agrees_with_lapack():
    g = np.random.default_rng(3).normal(size=(500, 3, 3))
    H = g @ g.transpose(0, 2, 1)
    lam, V = CO.jacobi_eigh3(H)
    want = np.linalg.eigvalsh(H)
    assert np.abs(lam - want).max() <= 1e-13 * np.abs(want).max()
    assert np.abs(np.einsum("nij,nj->ni", H, V[:, :, 0]) - lam[:, :1] * V[:, :, 0]).max() <= 1e-12 * np.abs(want).max()
    assert np.abs(np.einsum("nij,nik->njk", V, V) - np.eye(3)).max() <= 1e-14


def test_lattice_plane_is_exact():
    p = CO.lattice_plane()
    _, idx = CO.knn(p, p, 15, exclude_self=True)
    res = CO.estimate_normals(p, idx)
    assert (res["counts"] == 16).all() and not res["fallback"].any()
    assert np.array_equal(np.abs(res["normals"]), np.tile(np.float32([0, 0, 1]), (len(p), 1)))
    assert (res["eigenvalues"][:, 0] == 0.0).all() and (res["eigenvalues"][:, 1] > 0.0).all()


def test_fallbacks():
    p = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.3, 0.2, 0.9]])
    pad = np.full((4, 3), -1, dtype=np.int64)
    res = CO.estimate_normals(p, pad)                             # c = 1
    assert res["counts"].tolist() == [1] * 4 and np.array_equal(res["normals"], np.tile(np.float32([0, 0, 1]), (4, 1)))
    one = pad.copy(); one[:, 0] = (1, 0, 0, 0)
    res = CO.estimate_normals(p, one)                             # c = 2
    assert res["counts"].tolist() == [2] * 4 and res["fallback"].all() and (res["eigenvalues"] == 0).all()
    res = CO.estimate_normals(p, one, include_self=False)         # c = 1
    assert res["counts"].tolist() == [1] * 4 and res["fallback"].all()
    same = np.tile(np.float32([[0.25, -0.5, 0.125]]), (20, 1))    # coincident points: an all-zero covariance
    _, idx = CO.knn(same, same, 5, exclude_self=True)
    res = CO.estimate_normals(same, idx)
    assert (res["counts"] == 6).all() and res["fallback"].all() and np.array_equal(res["normals"], np.tile(np.float32([0, 0, 1]), (20, 1)))
    bad = p.copy(); bad[3, 1] = np.inf                            # a non-finite coordinate spoils every neighbourhood it is in
    full = np.array([[1, 2, 3], [0, 2, 3], [0, 1, -1], [0, 1, 2]], dtype=np.int64)
    res = CO.estimate_normals(bad, full)
    assert res["fallback"].tolist() == [True, True, False, True]
    assert np.array_equal(np.abs(res["normals"][2]), np.float32([0, 0, 1])) and res["eigenvalues"][2, 0] == 0.0      # three points of z = 0


def test_padding_and_self_slots_do_not_matter():
    p, _ = CO.sphere(600, seed=4)
    _, idx = CO.knn(p, p, 7, exclude_self=True)
    ref = CO.estimate_normals(p, idx)
    wide = np.full((600, 12), -1, dtype=np.int64)
    wide[:, [1, 2, 4, 5, 8, 9, 11]] = idx                         # the same slots in the same order, padding between them
    wide[:, 0] = np.arange(600); wide[::2, 3] = 600; wide[1::2, 6] = -(1 << 40)
    res = CO.estimate_normals(p, wide)
    for k in ("normals", "eigenvalues", "counts", "cov"):
        assert np.array_equal(res[k], ref[k]), k
    lam = np.linalg.eigvalsh(ref["cov"])
    assert np.abs(ref["eigenvalues"] - lam).max() <= 1e-12 * lam[:, 2].max()


def test_outlier_oracle():
    d = np.float32([[1, 4, 9], [4, 4, np.inf], [np.inf] * 3, [0.25, np.nan, 0.25], [100, 100, 100]])
    res = CO.outliers(d, 1.0)
    assert res["mean_dist"].tolist() == [2.0, 2.0, np.inf, 0.5, 10.0]
    fin = np.array([2.0, 2.0, 0.5, 10.0])
    assert res["mean"] == fin.mean() and res["std"] == pytest.approx(fin.std(), rel=1e-15)
    assert res["keep"].tolist() == [True, True, False, True, False] and res["kept_idx"].tolist() == [0, 1, 3]
    p, planted = CO.sheet_with_outliers()
    dist, _ = CO.knn(p, p, 16, exclude_self=True)
    res = CO.outliers(dist.astype(np.float32), 2.0)
    assert np.array_equal(np.flatnonzero(~res["keep"]), planted)
    margin = np.abs(res["mean_dist"] - res["threshold"]).min() / res["threshold"]
    print(f"planted outliers: threshold {res['threshold']:.4f}, closest row {margin:.3f} of it away")
    assert margin > 0.1


# ---- the PLY reader ------------------------------------------------------------------------------------------------------------------
def _write_bare_ply(path, pos, binary=True):
    head = "ply\nformat %s 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nend_header\n"
    with open(path, "wb") as f:
        f.write((head % ("binary_little_endian" if binary else "ascii", len(pos))).encode())
        if binary:
            f.write(np.asarray(pos, dtype="<f4").tobytes())
        else:
            f.write("".join("%.9g %.9g %.9g\n" % tuple(r) for r in pos).encode())


@pytest.mark.parametrize("binary", [True, False])
def test_read_ply_without_normals(tmp_path, binary):
    pos = np.random.default_rng(5).random((37, 3)).astype(np.float32)
    path = str(tmp_path / "scan.ply")
    _write_bare_ply(path, pos, binary)
    got, nrm = mesh.read_ply_points(path, require_normals=False)
    assert nrm is None and np.array_equal(got, pos)
    with pytest.raises(_lib.DudfError, match=r"scan\.ply has no normals: run preprocess\.py -pc, which estimates them"):
        mesh.read_ply_points(path)
    full = str(tmp_path / "full.ply")
    mesh.write_ply_points(full, pos, -pos)
    for kw in ({}, {"require_normals": False}, {"require_normals": True}):
        a, b = mesh.read_ply_points(full, **kw)
        assert np.array_equal(a, pos) and np.array_equal(b, -pos)


def test_preprocess_refuses_a_bare_cloud_only_when_told_not_to_estimate(tmp_path):
    from src.preprocess_mesh import preprocessPointCloud
    path = str(tmp_path / "scan.ply")
    _write_bare_ply(path, np.random.default_rng(6).random((50, 3)).astype(np.float32))
    with pytest.raises(_lib.DudfError, match="no normals"):
        preprocessPointCloud(str(tmp_path / "out"), path, surfacePoints=10, estimate_normals=False)
