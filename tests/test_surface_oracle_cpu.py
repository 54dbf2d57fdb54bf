# coding: utf-8
"""CPU: the numpy oracle of the device surface sampler (tests/surface_oracle.py) is pinned against the host sampler
`mesh.sample_surface`, which draws the same three random numbers per sample and differs only in how a face is chosen: there by a
floating-point cdf, here by 32-bit integer weights.  Plus what needs no device: weight-0 faces, refusals, the F-score at P = R = 0,
argument errors of the C entry points, the command line of cuantitative.py."""
import ctypes
import os

import numpy as np
import pytest

import surface_oracle as SO
from diffudf_amd import mesh

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def beetle():
    v, t = mesh.load_obj(os.path.join(HERE, "golden", "beetle.obj"))
    return mesh.normalize_vertices(v), t


def test_oracle_against_host_sampler(beetle):
    """The two samplers place the face boundaries at c_f / W and at cumsum(area)_f / sum(area): they differ by the truncation of
    the weights, at most F / 2^32 of the unit interval in total (F = 2 053: 4.8e-7), and by the rounding of the double cdf, so a
    sample changes face with a probability of about 1e-6.  Measured at 32 weight bits: the same face on 100 % of the rows at
    n = 1, 255, 256, 257 and 100 000 (W has 40 bits).  The condition is 99.9 %."""
    v, t = beetle
    for n in (1, 255, 256, 257, 100000):
        pos, nrm = mesh.sample_surface(v, t, n, seed=123)
        p, nm, face, fn, area = SO.sample_surface(v, t, n, seed=123)
        _, host_area = mesh.triangle_normals_areas(v, t)
        cdf = np.cumsum(host_area) / host_area.sum()
        host_face = np.minimum(np.searchsorted(cdf, mesh.synth.uniform01(123, 301, 0, n), side="right"), len(t) - 1)
        same = face == host_face
        print(f"n={n}: same face on {same.mean() * 100:.4f} % of rows; W has {int(SO.cumulative_weights(SO.face_terms(v, t)[1])[-1]).bit_length()} bits")
        assert same.mean() >= 0.999
        assert np.abs(p[same].astype(np.float64) - pos[same]).max() <= 1e-6
        assert np.abs(nm[same].astype(np.float64) - nrm[same]).max() <= 1e-6
        assert abs(area - host_area.sum()) <= 1e-13 * area
    assert p.dtype == np.float32 and nm.dtype == np.float32 and face.dtype == np.int64 and fn.shape == (len(t), 3)


def test_oracle_is_a_function_of_the_global_index(beetle):
    v, t = beetle
    whole = SO.sample_surface(v, t, 1000, seed=9)
    head, tail = SO.sample_surface(v, t, 400, seed=9), SO.sample_surface(v, t, 600, seed=9, start=400)
    for k in range(3):
        assert np.array_equal(whole[k], np.concatenate([head[k], tail[k]]))
    assert not np.array_equal(whole[0], SO.sample_surface(v, t, 1000, seed=10)[0])


def test_weight_zero_face_is_never_chosen():
    # face 1 is degenerate (two equal corners), face 3 has 2^-34 of the largest |e1 x e2|: both get weight 0
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [2.0 ** -34, 0, 0], [0, 0, 1]], dtype=np.float64)
    f = np.array([[0, 1, 2], [1, 3, 3], [1, 3, 2], [0, 4, 2], [0, 1, 5]], dtype=np.int64)
    c = SO.cumulative_weights(SO.face_terms(v, f)[1])
    assert c.tolist() == [2 ** 32, 2 ** 32, 2 ** 33, 2 ** 33, 3 * 2 ** 32]
    face = SO.sample_surface(v, f, 20000, seed=1)[2]
    assert set(face.tolist()) == {0, 2, 4}
    # also at the exact boundaries: t = c_0 belongs to face 2, not to the empty face 1; the last k to the last face
    u = np.array([[0.0, 0.5, 0.5], [1.0 / 3.0, 0.5, 0.5], [1.0 - 2.0 ** -53, 0.5, 0.5]])
    k = np.floor(u[:, 0] * SO.TWO53)
    assert [(int(ki) * int(c[-1])) >> 53 for ki in k] == [0, 2 ** 32 - 1, 3 * 2 ** 32 - 1]
    assert SO.sample_surface(v, f, 3, uniforms=u)[2].tolist() == [0, 0, 4]
    u[1, 0] = 3002399751580331 / SO.TWO53                       # k = ceil(2^53 / 3): the first k with t = 2^32 = c_0 exactly
    assert (3002399751580331 * int(c[-1])) >> 53 == 2 ** 32
    assert SO.sample_surface(v, f, 3, uniforms=u)[2].tolist() == [0, 2, 4]


def test_refusals_of_the_oracle():
    v = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], dtype=np.float64)
    with pytest.raises(ValueError, match="degenerate"):
        SO.sample_surface(v, np.array([[0, 1, 2], [0, 0, 1]]), 4)                  # collinear and collapsed: no area anywhere
    with pytest.raises(ValueError, match="no faces"):
        SO.sample_surface(v, np.zeros((0, 3), dtype=np.int64), 4)
    w = v.copy(); w[1, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        SO.sample_surface(w, np.array([[0, 1, 2]]), 4)
    with pytest.raises(ValueError, match="uniforms"):
        SO.sample_surface(np.eye(3), np.array([[0, 1, 2]]), 1, uniforms=np.array([[0.5, 1.0, 0.5]]))


def test_fscore_and_stats_oracle():
    from diffudf_amd import metrics
    assert SO.fscore(0.0, 0.0) == 0.0 and metrics.fscore(0.0, 0.0) == 0.0
    assert metrics.fscore(0.5, 1.0) == pytest.approx(2.0 / 3.0) and metrics.fscore(1.0, 1.0) == 1.0
    d = np.array([0.25, np.nan, 0.5, np.inf, 0.0], dtype=np.float32)
    s = SO.distance_stats(d, (0.25, 0.1, np.inf, -1.0))
    assert s["count_le"] == [2, 1, 4, 0] and s["nan"] == 1 and s["max"] == np.inf
    s = SO.distance_stats(d[:3], ())
    assert s["count_le"] == [] and s["nan"] == 1 and s["max"] == 0.5 and s["sum"] == 0.75 and s["sum_sq"] == 0.3125
    assert SO.distance_stats(np.zeros(0, np.float32), (1.0,)) == {"count_le": [0], "nan": 0, "max": 0.0, "sum": 0.0, "sum_sq": 0.0}


def test_entry_points_refuse_before_any_device_call():
    from diffudf_amd import _lib
    lib = _lib.load()
    NULL = ctypes.c_void_p(0)
    one = ctypes.c_void_p(256)                                  # never dereferenced: every call below returns on its arguments
    assert lib.dudf_mesh_sample_surface_workspace(0) == 0 and lib.dudf_mesh_sample_surface_workspace(1 << 31) == 0
    assert lib.dudf_mesh_sample_surface_workspace(1) % 256 == 0 and lib.dudf_mesh_sample_surface_workspace(1) > 0
    assert lib.dudf_mesh_sample_surface_workspace(300000) > lib.dudf_mesh_sample_surface_workspace(1)
    args = lambda F, n=1, start=0: (one, 3, one, F, start, n, 1, NULL, one, NULL, NULL, NULL, NULL, NULL, 0, NULL)   # noqa: E731
    assert lib.dudf_mesh_sample_surface(*args(0)) == -1
    assert lib.dudf_mesh_sample_surface(*args(1, n=-1)) == -1
    assert lib.dudf_mesh_sample_surface(*args(1, start=-1)) == -1
    assert lib.dudf_mesh_sample_surface(*args(1 << 31)) == -4
    assert lib.dudf_mesh_sample_surface(*args(1)) == -2         # no workspace
    taus = (ctypes.c_double * 17)(*range(17))
    assert lib.dudf_distance_stats_workspace_bytes(0) == 256
    assert lib.dudf_distance_stats(one, 1, taus, 17, one, one, one, one, 256, NULL) == -4
    assert lib.dudf_distance_stats(one, 1, taus, -1, one, one, one, one, 256, NULL) == -4
    assert lib.dudf_distance_stats(one, -1, taus, 1, one, one, one, one, 256, NULL) == -1
    assert lib.dudf_distance_stats(one, 1, taus, 1, one, one, one, NULL, 0, NULL) == -2
    assert _lib.ABI_VERSION == 8 and int(lib.dudf_abi_version()) == 8


def test_cuantitative_command_line_and_header():
    import cuantitative
    assert cuantitative.parse_args([]) == ('data/deepfashion/', 'results/df_subset/', 0, 0, (0.005, 0.01))
    assert cuantitative.parse_args(['d/', 'o/', '2']) == ('d/', 'o/', 2, 0, (0.005, 0.01))
    assert cuantitative.parse_args(['d/', 'o/', '1', '--surface-samples', '1000', '--fscore-taus', '0.02,0.1']) == ('d/', 'o/', 1, 1000, (0.02, 0.1))
    assert cuantitative.parse_args(['d/', '--surface-samples', '7']) == ('d/', 'results/df_subset/', 0, 7, (0.005, 0.01))
    h = cuantitative.surface_header((0.005, 0.01)).split(',')
    assert h[0] == 'mesh' and len(h) == 1 + 2 * (6 + 3 * 2)
    assert h[1:13] == ['accuracy_CAP', 'completeness_CAP', 'chamfer_l1_CAP', 'chamfer_l2_CAP', 'hausdorff_CAP', 'precision@0.005_CAP',
                       'precision@0.01_CAP', 'recall@0.005_CAP', 'recall@0.01_CAP', 'fscore@0.005_CAP', 'fscore@0.01_CAP', 'NC_CAP']
    assert h[13:] == [c[:-3] + 'MU' for c in h[1:13]]
    assert cuantitative.HEADER == 'mesh,time,L1CD_CAP,L2CD_CAP,NC_CAP,L1CD_MU,L2CD_MU,NC_MU'
    assert all(np.isnan(x) for x in cuantitative.surface_fields(None, None, None, 10, (0.1,), 0)) and \
        len(cuantitative.surface_fields(None, None, None, 10, (0.1,), 0)) == 9
