# coding: utf-8
"""CPU: Lewiner marching cubes of a SIGNED volume on the host (`dudf_mc_lewiner_run` behind `marching_cubes.marching_cubes_lewiner`).

The triangulation code is the one tests/test_meshudf.py holds bit for bit to the reference's extension; what is new is the raster
driver round it, so the checks here do not need the tables to know the answer: a table-free oracle of the vertex set, the
reference-pinned MeshUDF extraction on the same surfaces, and the geometry of closed smooth surfaces.  Parity with scikit-image's
`marching_cubes` itself is unpinned (it is not installed, and the reference's extension has no signed entry point).  The tables come
from tests/golden/g10_meshudf.npz."""
import os
from collections import Counter

import numpy as np
import pytest

from diffudf_amd import marching_cubes as M

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def luts():
    z = np.load(os.path.join(HERE, "golden", "g10_meshudf.npz"))
    return {k[4:]: z[k] for k in z.files if k.startswith("lut_")}


def grid(shape):
    return np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")


def sphere(shape, centre, r):
    g = grid(shape)
    return np.sqrt(sum((a - c) ** 2 for a, c in zip(g, centre))) - r


def torus(shape, centre, R, r):
    g = grid(shape)
    q = np.sqrt((g[1] - centre[1]) ** 2 + (g[2] - centre[2]) ** 2) - R
    return np.sqrt(q ** 2 + (g[0] - centre[0]) ** 2) - r


# ---- 1. table-free vertex oracle -------------------------------------------------------------------------------------------------
def crossed_edge_vertices(vol, level):
    """(x, y, z) float32 of every grid edge whose ends lie on different sides (value - level > 0 or not): i + w2 / (w1 + w2),
    w = 1 / (2^-52 + |v|), in fp64, rounded once."""
    v = vol.astype(np.float32).astype(np.float64) - level
    out = []
    for axis in range(3):
        a = np.moveaxis(v, axis, 0)
        v1, v2 = a[:-1], a[1:]
        idx = np.argwhere((v1 > 0) != (v2 > 0))
        w1, w2 = 1.0 / (EPS + np.abs(v1[tuple(idx.T)])), 1.0 / (EPS + np.abs(v2[tuple(idx.T)]))
        pos = idx.astype(np.float64)
        pos[:, 0] += w2 / (w1 + w2)
        order = [axis] + [k for k in range(3) if k != axis]          # columns of `pos` as volume axes
        zyx = np.empty_like(pos)
        for col, ax in enumerate(order):
            zyx[:, ax] = pos[:, col]
        out.append(zyx[:, ::-1])
    return np.concatenate(out).astype(np.float32)


def rows_sorted(a):
    a = np.asarray(a)
    return a[np.lexsort(a.T[::-1])]


ORACLE_CASES = {
    "sphere": (lambda: sphere((14, 15, 16), (6.3, 7.1, 7.7), 4.6), 0.0),
    "sphere_level": (lambda: sphere((13, 13, 13), (6.2, 5.9, 6.4), 3.0), 1.25),
    "torus": (lambda: torus((12, 20, 21), (5.4, 9.6, 10.2), 5.5, 2.3), 0.0),
    "noise": (lambda: np.random.default_rng(11).normal(size=(9, 10, 11)), 0.0),
    "noise_level": (lambda: np.random.default_rng(12).normal(size=(9, 10, 11)), -0.3),
}


@pytest.mark.parametrize("name", sorted(ORACLE_CASES))
def test_vertices_are_the_crossed_edges(luts, name):
    make, level = ORACLE_CASES[name]
    vol = make().astype(np.float32)
    v, f, n, vals = M.marching_cubes_sdf(vol, level, luts)
    assert v.dtype == np.float32 and f.dtype == np.int32 and f.size % 3 == 0 and f.min() >= 0 and f.max() == len(v) - 1
    whole = (v == np.floor(v)).sum(axis=1)
    on_edge, centre = v[whole >= 2], v[whole < 2]
    want = crossed_edge_vertices(vol, level)
    assert len(on_edge) == len(want)
    assert np.array_equal(rows_sorted(on_edge), rows_sorted(want))
    frac = centre - np.floor(centre)                       # every other vertex is a centre vertex: strictly inside its cube
    assert np.all((frac > 0) & (frac < 1))
    hi = np.array(vol.shape[::-1]) - 1
    assert np.all(centre > 0) and np.all(centre < hi)
    if name.startswith("noise"):
        assert len(centre) > 0                             # noise reaches the tilings with a centre vertex


# ---- 2. against the reference-pinned MeshUDF extraction --------------------------------------------------------------------------
def shapes_for_meshudf():
    rng = np.random.default_rng(5)
    out = []
    for k in range(10):
        N = int(rng.integers(10, 34))
        x = np.linspace(-1.0, 1.0, N)
        Z, Y, X = np.meshgrid(x, x, x, indexing="ij")
        c = rng.uniform(-0.05, 0.05, 3) + 0.0137
        dz, dy, dx = Z - c[0], Y - c[1], X - c[2]
        if k % 2 == 0:
            r = np.sqrt(dx * dx + dy * dy + dz * dz)
            sd = r - rng.uniform(0.45, 0.7)
            g = np.stack([dz, dy, dx], -1) / r[..., None]
        else:
            R, rr = rng.uniform(0.5, 0.6), rng.uniform(0.2, 0.28)
            rho = np.sqrt(dx * dx + dy * dy)
            q = rho - R
            d = np.sqrt(q * q + dz * dz)
            sd = d - rr
            g = np.stack([dz / d, q / d * dy / rho, q / d * dx / rho], -1)
        out.append((f"{'sphere' if k % 2 == 0 else 'torus'}_{N}", sd.astype(np.float32), g.astype(np.float32), 2 if k % 2 == 0 else 0))
    return out


def euler(v, f):
    e = {tuple(sorted((int(t[a]), int(t[b])))) for t in f for a, b in ((0, 1), (1, 2), (2, 0))}
    return len(v) - len(e) + len(f)


def triangle_set(v, f):
    key = [tuple(r) for r in v.tolist()]
    return Counter(frozenset(key[i] for i in t) for t in f.tolist())


def describe_cube(tri, sd, luts):
    """The cube a triangle lies in and its Lewiner case, for the message of a failed comparison (vertices in z-y-x order)."""
    pts = np.array(sorted(tri))
    z, y, x = np.floor(pts.min(axis=0) + 1e-9).astype(int)
    z, y, x = min(z, sd.shape[0] - 2), min(y, sd.shape[1] - 2), min(x, sd.shape[2] - 2)
    kx, ky, kz = (0, 1, 1, 0, 0, 1, 1, 0), (0, 0, 1, 1, 0, 0, 1, 1), (0, 0, 0, 0, 1, 1, 1, 1)
    index = sum(1 << c for c in range(8) if sd[z + kz[c], y + ky[c], x + kx[c]] > 0)
    return f"cube (z, y, x) = ({z}, {y}, {x}), sign index {index}, case {int(luts['CASES'][index, 0])}, config {int(luts['CASES'][index, 1])}"


def test_same_surface_as_meshudf(luts):
    for name, sd, g, chi in shapes_for_meshudf():
        udf = np.abs(sd)
        vec = (-g * np.sign(sd)[..., None]).astype(np.float32)
        vu, fu, _, _ = M.udf_mc_lewiner(udf, vec, luts=luts)
        vs, fs, _, _ = M.marching_cubes_lewiner(sd, 0.0, luts=luts)
        assert np.array_equal(rows_sorted(vu), rows_sorted(vs)), name
        assert euler(vs, fs) == chi, name
        tu, ts = triangle_set(vu, fu), triangle_set(vs, fs)
        if tu != ts:
            odd = next(iter((tu - ts) + (ts - tu)))
            raise AssertionError(f"{name}: {sum((tu - ts).values())} MeshUDF triangles are not in the signed mesh and "
                                 f"{sum((ts - tu).values())} the other way round; first: {describe_cube(odd, sd, luts)}")


# ---- 3. smooth closed surfaces ---------------------------------------------------------------------------------------------------
def signed_volume(v, f):
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def area(v, f):
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return float(0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1).sum())


def closed_cases():
    N = 40
    h = 2.0 / (N - 1)
    x = np.linspace(-1.0, 1.0, N)
    Z, Y, X = np.meshgrid(x, x, x, indexing="ij")
    r0, c0 = 0.61, np.array([0.013, -0.021, 0.017])
    sph = np.sqrt((Z - c0[0]) ** 2 + (Y - c0[1]) ** 2 + (X - c0[2]) ** 2) - r0
    R, rr = 0.55, 0.23
    tor = np.sqrt((np.sqrt((Y - c0[1]) ** 2 + (X - c0[2]) ** 2) - R) ** 2 + (Z - c0[0]) ** 2) - rr
    r2, d = 0.42, 0.5
    two = np.minimum(np.sqrt(Z ** 2 + Y ** 2 + (X - d / 2) ** 2), np.sqrt(Z ** 2 + Y ** 2 + (X + d / 2) ** 2)) - r2
    lens = np.pi * (4 * r2 + d) * (2 * r2 - d) ** 2 / 12
    return h, {"sphere": (sph, 4 / 3 * np.pi * r0 ** 3, 2, c0), "torus": (tor, 2 * np.pi ** 2 * R * rr ** 2, 0, None),
               "two_spheres": (two, 2 * 4 / 3 * np.pi * r2 ** 3 - lens, 2, None)}


@pytest.mark.parametrize("name", ["sphere", "torus", "two_spheres"])
def test_closed_smooth_surfaces(luts, name):
    h, cases = closed_cases()
    sd, volume, chi, centre = cases[name]
    sd = sd.astype(np.float32)
    v, f, n, _ = M.marching_cubes_lewiner(sd, 0.0, spacing=(h, h, h), luts=luts)
    directed = Counter((int(t[a]), int(t[b])) for t in f for a, b in ((0, 1), (1, 2), (2, 0)))
    assert all(directed[(b, a)] == k for (a, b), k in directed.items())        # closed and consistently oriented
    assert euler(v, f) == chi
    vol = signed_volume(v, f)
    # marching cubes places the surface within one cell of the true one: the volume between them is at most ~ h * area (3 h allowed)
    assert abs(abs(vol) - volume) <= 3 * h * area(v, f), (vol, volume)
    va, fa, _, _ = M.marching_cubes_lewiner(sd, 0.0, spacing=(h, h, h), gradient_direction="ascent", luts=luts)
    assert np.array_equal(va, v) and np.array_equal(fa, f[:, ::-1])
    assert signed_volume(va, fa) == pytest.approx(-vol, rel=1e-12)
    if centre is not None:                                                     # normals of the sphere: radial, one sign throughout
        radial = (v - 1.0) - centre
        cos = np.einsum("ij,ij->i", radial / np.linalg.norm(radial, axis=1, keepdims=True), n.astype(np.float64))
        assert np.all(np.abs(cos) > 0.95)
        assert np.all(cos > 0) or np.all(cos < 0)
        # recorded in DESIGN.md §3.5a: the sums are of v(lower corner) - v(upper corner), so the normals point DOWN the field,
        # towards the inside of a signed distance function that is negative inside
        assert np.all(cos < 0)


# ---- 4. every tiling uses exactly the crossed edges of its cube --------------------------------------------------------------------
TILINGS_OF_CASE = {
    1: ["TILING1"], 2: ["TILING2"], 3: ["TILING3_1", "TILING3_2"], 4: ["TILING4_1", "TILING4_2"], 5: ["TILING5"],
    6: ["TILING6_1_1", "TILING6_1_2", "TILING6_2"], 7: ["TILING7_1", "TILING7_2", "TILING7_3", "TILING7_4_1", "TILING7_4_2"],
    8: ["TILING8"], 9: ["TILING9"], 10: ["TILING10_1_1", "TILING10_1_1_", "TILING10_1_2", "TILING10_2", "TILING10_2_"],
    11: ["TILING11"], 12: ["TILING12_1_1", "TILING12_1_1_", "TILING12_1_2", "TILING12_2", "TILING12_2_"],
    13: ["TILING13_1", "TILING13_1_", "TILING13_2", "TILING13_2_", "TILING13_3", "TILING13_3_", "TILING13_4", "TILING13_5_1",
         "TILING13_5_2"], 14: ["TILING14"]}


def test_every_tiling_uses_exactly_the_crossed_edges(luts):
    """The device kernel numbers an edge vertex in the lowest-raster cube round the edge: that cube must USE the edge.  So must
    every other cube round it (normals are gathered over them).  Holds when each triangle list names every crossed edge of its
    sign index, and no other (12 = the centre vertex aside)."""
    corner = {(0, 0, 0): 0, (1, 0, 0): 1, (1, 1, 0): 2, (0, 1, 0): 3, (0, 0, 1): 4, (1, 0, 1): 5, (1, 1, 1): 6, (0, 1, 1): 7}
    ex, ey, ez = luts["EDGESRELX"], luts["EDGESRELY"], luts["EDGESRELZ"]
    ends = [(corner[(int(ex[e, 0]), int(ey[e, 0]), int(ez[e, 0]))], corner[(int(ex[e, 1]), int(ey[e, 1]), int(ez[e, 1]))]) for e in range(12)]
    seen_cases, checked = set(), 0
    for index in range(256):
        c, config = int(luts["CASES"][index, 0]), int(luts["CASES"][index, 1])
        crossed = {e for e, (a, b) in enumerate(ends) if (index >> a & 1) != (index >> b & 1)}
        if c <= 0:
            assert not crossed and index in (0, 255)
            continue
        seen_cases.add(c)
        for name in TILINGS_OF_CASE[c]:
            t = luts[name]
            rows = t[config].reshape(-1, t.shape[-1]) if t.ndim == 3 else t[config][None]
            for sub, row in enumerate(rows):
                used = set(int(e) for e in row)
                assert used - {12} == crossed, (index, c, config, name, sub)
                assert len(row) % 3 == 0 and max(used) <= 12 and min(used) >= 0
                checked += 1
    assert seen_cases == set(range(1, 15)) and checked >= 254             # at least one list per sign index with a surface
    assert luts["SUBCONFIG13"].min() >= -1 and luts["SUBCONFIG13"].max() == 45


# ---- 5. wrapper contract --------------------------------------------------------------------------------------------------------
def test_wrapper_contract(luts):
    vol = sphere((8, 8, 8), (3.4, 3.5, 3.6), 2.2).astype(np.float32)
    with pytest.raises(ValueError, match="3D numpy array"):
        M.marching_cubes_lewiner(vol[0], 0.0, luts=luts)
    with pytest.raises(ValueError, match="3D numpy array"):
        M.marching_cubes_lewiner(vol.tolist(), 0.0, luts=luts)
    with pytest.raises(ValueError, match="at least 2x2x2"):
        M.marching_cubes_lewiner(vol[:1], 0.0, luts=luts)
    with pytest.raises(ValueError, match="Surface level must be within volume data range"):
        M.marching_cubes_lewiner(vol, 100.0, luts=luts)
    with pytest.raises(ValueError, match="Surface level must be within volume data range"):
        M.marching_cubes_lewiner(vol, -100.0, luts=luts)
    with pytest.raises(ValueError, match="three floats"):
        M.marching_cubes_lewiner(vol, 0.0, spacing=(1, 1), luts=luts)
    with pytest.raises(ValueError, match="step_size must be at least one"):
        M.marching_cubes_lewiner(vol, 0.0, step_size=0, luts=luts)
    with pytest.raises(ValueError, match="same shape"):
        M.marching_cubes_lewiner(vol, 0.0, mask=np.ones((2, 2, 2), bool), luts=luts)
    with pytest.raises(ValueError, match="gradient_direction"):
        M.marching_cubes_lewiner(vol, 0.0, gradient_direction="sideways", luts=luts)
    for kw in ({"step_size": 2}, {"mask": np.ones(vol.shape, bool)}, {"use_classic": True}, {"allow_degenerate": False}):
        with pytest.raises(NotImplementedError):
            M.marching_cubes_lewiner(vol, 0.0, luts=luts, **kw)
    with pytest.raises(RuntimeError, match="No surface found"):
        M.marching_cubes_lewiner(np.ones((4, 4, 4), np.float32), 1.0, luts=luts)       # level in range, nothing above it
    # level None = mid-range; z-y-x order; spacing
    v0, f0, n0, _ = M.marching_cubes_lewiner(vol, luts=luts)
    v1, f1, _, _ = M.marching_cubes_lewiner(vol, 0.5 * (float(vol.min()) + float(vol.max())), luts=luts)
    assert np.array_equal(v0, v1) and np.array_equal(f0, f1) and f0.shape[1] == 3
    raw, fr, _, _ = M.marching_cubes_sdf(vol, 0.5 * (float(vol.min()) + float(vol.max())), luts)
    assert np.array_equal(v0, raw[:, ::-1]) and np.array_equal(f0, fr.reshape(-1, 3)[:, ::-1])
    v2, _, n2, _ = M.marching_cubes_lewiner(vol, luts=luts, spacing=(0.5, 2.0, 3.0))
    assert v2.dtype == np.float64 and np.array_equal(v2, v0 * np.r_[0.5, 2.0, 3.0]) and np.array_equal(n2, n0)
    assert np.allclose(np.linalg.norm(n0.astype(np.float64), axis=1), 1.0, atol=1e-6)


def test_lattice_zeros_and_the_smallest_volume(luts):
    # an integer-valued field: the level passes THROUGH grid points, whose vertices land on them exactly
    z = np.arange(7, dtype=np.float32)[:, None, None] - 3.0 + np.zeros((7, 5, 6), np.float32)
    v, f, _, _ = M.marching_cubes_lewiner(z, 0.0, luts=luts)
    assert len(f) > 0 and np.all(v[:, 0] == 3.0)
    assert np.all(v == np.floor(v))
    one = np.zeros((2, 2, 2), np.float32); one[0, 0, 0] = 1.0
    v, f, n, vals = M.marching_cubes_lewiner(one, 0.5, luts=luts)
    assert v.shape == (3, 3) and f.shape == (1, 3) and np.all(vals == 1.0)
    assert sorted(map(tuple, v.tolist())) == [(0.0, 0.0, 0.5), (0.0, 0.5, 0.0), (0.5, 0.0, 0.0)]


# ---- 6. the Python surface that needs no GPU -------------------------------------------------------------------------------------
def test_render_mc_surface(luts, capsys):
    import torch
    from src.render_mc import TriangleSoup, convert_sdf_samples_to_ply, gen_sdf_coordinate_grid, get_mesh_sdf  # noqa: F401
    from src.marching_cubes._marching_cubes_lewiner import marching_cubes_lewiner  # noqa: F401
    n = np.array([[0.0, 0.0, 1.0]] * 3)
    soup = TriangleSoup(np.eye(3), np.array([[0, 1, 2]]), vertex_normals=n)
    assert np.array_equal(soup.vertex_normals, n) and soup.vertex_normals.dtype == np.float64
    N, voxel = 5, 0.5
    s = gen_sdf_coordinate_grid(N, voxel, torch.device("cpu"))
    assert s.shape == (N ** 3, 4) and s.dtype == torch.float32 and float(s[:, 3].abs().max()) == 0.0
    i = np.arange(N ** 3)
    # the reference divides the int64 index in floating point before the modulo (`/`, not `//`): columns 0 and 1 carry fractions
    want = np.stack([((i / N) / N) % N, (i / N) % N, i % N], 1).astype(np.float32) * np.float32(voxel) - 1.0
    assert np.allclose(s[:, :3].numpy(), want, atol=1e-6)
    # a CPU tensor goes through the host library; offset / scale as the reference applies them
    vol = torch.from_numpy(sphere((9, 9, 9), (4.2, 3.9, 4.1), 2.7).astype(np.float32))
    pts, faces, normals, values = convert_sdf_samples_to_ply(vol, [-1, -1, -1], 0.25, offset=np.array([0.5, 0.0, -0.5]), scale=2.0, luts=luts)
    v, f, nn, vals = M.marching_cubes_lewiner(vol.numpy(), 0.0, spacing=[0.25] * 3, luts=luts)
    assert np.array_equal(pts, (v - 1.0) / 2.0 - np.array([0.5, 0.0, -0.5])) and np.array_equal(faces, f) and np.array_equal(normals, nn)
    capsys.readouterr()
    pts, faces, normals, values = convert_sdf_samples_to_ply(torch.ones(3, 3, 3), [-1, -1, -1], 1.0, luts=luts)
    assert "Surface level must be within volume data range." in capsys.readouterr().out
    assert pts.shape == (0, 3) and faces.shape == (0, 3) and normals.shape == (0, 3) and values.shape == (0,)


def test_device_entry_points_refuse_bad_arguments(luts):
    """The checks of dudf_mc_lewiner_* and dudf_grid_values run before the first HIP call (no GPU needed): the "device" pointers
    are a host address that is never read."""
    import ctypes
    from diffudf_amd import _lib
    lib = _lib.load()
    arena = ctypes.create_string_buffer(1 << 16)
    P = ctypes.c_void_p((ctypes.addressof(arena) + 255) // 256 * 256)
    data, offs, dims = M._pack_luts(luts)
    o, d = ctypes.c_void_p(offs.ctypes.data), ctypes.c_void_p(dims.ctypes.data)
    nb = lib.dudf_mc_lewiner_workspace_bytes(5, 6, 7)
    assert nb >= 4 * 5 * 6 * 4 and lib.dudf_mc_lewiner_workspace_bytes(1, 6, 7) == 0 and lib.dudf_mc_lewiner_workspace_bytes(5, 6, 4096) == 0
    count = lambda nz=5, luts_=P, n=51, ws=P, nbytes=nb, dims_=d: lib.dudf_mc_lewiner_count(P, nz, 6, 7, 0.0, luts_, o, dims_, n, P, ws, nbytes, None)  # noqa: E731
    assert count(nz=1) == -1 and count(luts_=None) == -1 and count(n=50) == -1
    assert count(ws=None) == -2 and count(nbytes=nb - 1) == -2
    big = dims.copy(); big[3 * 3] = 4096                                 # tables that do not fit the kernel's 18 KiB of LDS
    assert count(dims_=ctypes.c_void_p(big.ctypes.data)) == -1
    assert lib.dudf_mc_lewiner_emit(P, 5, 6, 7, 0.0, P, o, d, 51, P, P, P, None, P, nb, None) == -1      # every output is required
    cfg = _lib.NetCfg(3, 2, 32, 30.0)
    need = lib.dudf_workspace_bytes_query(ctypes.byref(cfg), 8, 0)
    gv = lambda start, count_, c=cfg: lib.dudf_grid_values(ctypes.byref(c), P, 4, start, count_, P, P, need, None)  # noqa: E731
    assert gv(0, 0) == 0 and gv(-1, 8) == -1 and gv(60, 8) == -1 and gv(0, 8, _lib.NetCfg(3, 2, 100, 30.0)) == -1
    assert lib.dudf_grid_values(ctypes.byref(cfg), P, 4, 0, 8, P, None, need, None) == -2
