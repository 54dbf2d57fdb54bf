# coding: utf-8
"""GPU: the brick-sparse narrow band.
  1. the selection equals the numpy oracle (slot table, both id lists, both counts) at sizes of one brick, a partial brick,
     m % B == 0 and != 0 and more than one workgroup of bricks, with a planted NaN and a corner exactly on the bound;
  2. sparse CAP-UDF on `SparseFields.from_dense` of the analytic fields equals the dense extractor bit for bit (tests/
     test_sparse_mc_cpu.py shows that the candidate bricks cover every active cell there, so equality has no exceptions);
  3. the brick fields are `extract_fields`' fields at the same points, the eigenvector fallback included;
  4. end to end on a network whose field is provably 1-Lipschitz (a plane through a one-live-unit SIREN);
  5. 1025^3, which the dense path cannot reasonably reach: memory below the dense df array alone, every vertex on the plane;
  6. `generate_mc(sparse=True)` writes that mesh; without the key the dense file is what the dense functions write."""
import os

import numpy as np
import pytest
import torch

import sparsegrid_oracle as S
from test_capudf import analytic_fields
from test_fields_gpu import make_model

pytestmark = pytest.mark.gpu

PLANE_N = np.array([0.36, 0.48, 0.8])
PLANE_C0 = 0.137


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def tri_rows(v, t):
    """The triangle multiset as sorted (T, 9) float64 rows of verts[tris]."""
    v = v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
    t = t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    rows = v[t].reshape(len(t), 9)
    return rows[np.lexsort(rows.T[::-1])]


def cell_set(c):
    return {tuple(r) for r in c.cpu().numpy().tolist()}


_dense = {}


def dense_fields(kind, N):
    """Analytic fields on the device, made once and left unchanged."""
    if (kind, N) not in _dense:
        ndf, vec = analytic_fields(N, kind)
        _dense[(kind, N)] = (ndf, vec, dev(ndf), dev(vec))
    return _dense[(kind, N)]


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,B", [(2, 4), (5, 4), (9, 8), (20, 8), (33, 4), (33, 8), (65, 8), (129, 8)])
def test_selection_equals_the_oracle(N, B):
    """129 / 8: 17^3 = 4913 lattice bricks are 20 workgroups; 2 / 4 is one brick, 5 / 4 and 9 / 8 have m % B == 0 (a storage brick
    that holds no cell), 20 / 8 a partial brick."""
    from diffudf_amd import hip_ops
    m, nb, nl = S.dims(N, B)
    ix = S.lattice_indices(N, B)
    for kind in ("sphere", "sheet"):
        coarse = dense_fields(kind, N)[0][np.ix_(ix, ix, ix)]
        for thr in (0.008, 2.0 * (2.0 / (N - 1))):
            bnd = S.bound(N, B, thr, 1.25)
            slot_o, stored_o, cand_o = S.select(coarse, N, B, bnd)
            slot, stored, cand = hip_ops.sparse_select(dev(coarse), N, B, bnd)
            assert slot.shape == (nl, nl, nl) and slot.dtype == torch.int32 and stored.dtype == torch.int32
            assert np.array_equal(slot.cpu().numpy(), slot_o)
            assert np.array_equal(stored.cpu().numpy(), stored_o) and np.array_equal(cand.cpu().numpy(), cand_o)
    print(f"select {N}/{B}: {len(cand_o)} candidates, {len(stored_o)} stored of {nl ** 3}")


def test_selection_nan_and_equality():
    from diffudf_amd import hip_ops
    N, B = 33, 8
    m, nb, nl = S.dims(N, B)
    bnd = 0.25
    coarse = np.full((nb + 1,) * 3, 1.0, dtype=np.float32)
    coarse[0, 0, 0] = np.float32(bnd)                     # exactly the bound: selected
    coarse[4, 4, 4] = np.nan                              # a NaN corner: selected
    coarse[2, 0, 4] = np.nextafter(np.float32(bnd), np.float32(1))      # one float above: not selected
    slot_o, stored_o, cand_o = S.select(coarse, N, B, bnd)
    assert len(cand_o) == 2 and len(stored_o) == 16
    slot, stored, cand = hip_ops.sparse_select(dev(coarse), N, B, bnd)
    assert np.array_equal(slot.cpu().numpy(), slot_o)
    assert np.array_equal(stored.cpu().numpy(), stored_o) and np.array_equal(cand.cpu().numpy(), cand_o)
    none = hip_ops.sparse_select(dev(np.full((nb + 1,) * 3, 1.0, dtype=np.float32)), N, B, bnd)
    assert int((none[0] >= 0).sum()) == 0 and none[1].numel() == 0 and none[2].numel() == 0


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sheet", "sphere"])
@pytest.mark.parametrize("N,B", [(20, 8), (33, 8), (65, 8), (33, 4)])
def test_sparse_cap_equals_dense_cap_bit_for_bit(kind, N, B):
    from diffudf_amd import hip_ops
    from src.render_mc import SparseFields
    ndf, vec, d_ndf, d_vec = dense_fields(kind, N)
    m, nb, nl = S.dims(N, B)
    for thr in (0.008, 2.0 * (2.0 / (N - 1))):
        f = SparseFields.from_dense(d_ndf, d_vec, threshold=thr, brick=B, lipschitz=1.25)
        slot_o, stored_o, cand_o = S.select(ndf[np.ix_(*[S.lattice_indices(N, B)] * 3)], N, B, S.bound(N, B, thr, 1.25))
        assert np.array_equal(f.stored_ids.cpu().numpy(), stored_o) and np.array_equal(f.candidate_ids.cpu().numpy(), cand_o)
        df_o, vec_o = S.gather(ndf, vec, stored_o, N, B)
        assert np.array_equal(f.df.cpu().numpy(), df_o) and np.array_equal(f.vec.cpu().numpy(), vec_o)
        v, t, c, counts = f.extract(want_cells=True, want_counts=True)
        vd, td, cd = hip_ops.capudf_extract(d_ndf, d_vec, threshold=thr, want_cells=True)
        assert counts == (len(cd), len(vd), len(td)) and len(cd) > 0
        assert (len(c), len(v), len(t)) == counts
        assert cell_set(c) == cell_set(cd)
        assert np.array_equal(tri_rows(v, t), tri_rows(vd, td))
        # emission order: candidate bricks ascending, cells in local (i, j, k) order inside each
        cc = c.cpu().numpy()
        brick = ((cc[:, 0] // B) * nl + cc[:, 1] // B) * nl + cc[:, 2] // B
        local = ((cc[:, 0] % B) * B + cc[:, 1] % B) * B + cc[:, 2] % B
        key = brick * B ** 3 + local
        assert np.all(np.diff(key) > 0) and set(brick.tolist()) <= set(cand_o.tolist())
        v2, t2, c2 = f.extract(want_cells=True)
        assert torch.equal(v, v2) and torch.equal(t, t2) and torch.equal(c, c2)
        # gather / scatter
        a, b = f.to_dense()
        ao, bo = S.scatter(df_o, vec_o, stored_o, N, B)
        assert np.array_equal(a.cpu().numpy(), ao, equal_nan=True) and np.array_equal(b.cpu().numpy(), bo, equal_nan=True)
    print(f"sparse CAP {kind} {N}/{B}: {counts} cells / vertices / triangles from {len(cand_o)} candidate bricks")


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden,N,B", [([64] * 3, 20, 8), ([256] * 8, 20, 8), ([64] * 3, 13, 4), ([256] * 8, 13, 4)])
def test_brick_fields_are_the_grids_fields(hidden, N, B):
    from src.render_mc import extract_fields, extract_fields_sparse
    model, _ = make_model(hidden, 5)
    d = torch.device("cuda:0")
    df, vecs = extract_fields(model, None, N, "tanh", d, 100.0)
    f = extract_fields_sparse(model, None, N, "tanh", d, 100.0, brick=B, lipschitz=1e9)
    m, nb, nl = S.dims(N, B)
    assert f.stored_ids.numel() == nl ** 3 and f.candidate_ids.numel() == nb ** 3
    a, b = f.to_dense()                                   # only in-grid points: the padding of partial bricks is never compared
    assert not torch.isnan(a).any() and not torch.isnan(b).any()
    scale = float(df.abs().max())
    e_df, e_vec = float((a - df).abs().max()), float((b - vecs).abs().max())
    print(f"brick fields {len(hidden)}x{hidden[0]} {N}/{B}: |d df| {e_df:.2e} (bound {2e-6 * scale:.2e}), |d vec| {e_vec:.2e}")
    assert e_df <= 2e-6 * scale and e_vec < 2e-5
    # small chunks: several calls, a shorter last one
    g = extract_fields_sparse(model, None, N, "tanh", d, 100.0, brick=B, lipschitz=1e9, chunk=3 * B ** 3 + 1)
    assert float((g.df - f.df).abs().max()) <= 2e-6 * scale and float((g.vec - f.vec).abs().max()) < 2e-5


def test_brick_fields_eigenvector_fallback():
    from src.render_mc import extract_fields, extract_fields_sparse
    N, B = 10, 4
    model, _ = make_model([64] * 3, 5, out_scale=1e-20)
    d = torch.device("cuda:0")
    _, vecs = extract_fields(model, None, N, "tanh", d, 100.0)
    f = extract_fields_sparse(model, None, N, "tanh", d, 100.0, brick=B, lipschitz=1e9)
    _, b = f.to_dense()
    nrm = b.norm(dim=-1)
    dot = (b * vecs).sum(-1).abs()
    print(f"fallback {N}/{B}: | |v| - 1 | {float((nrm - 1).abs().max()):.2e}, min |dot| {float(dot.min()):.6f}")
    assert float((nrm - 1).abs().max()) < 1e-4 and float(dot.min()) >= 1 - 1e-3
    assert float((f.vec.reshape(-1, 3).norm(dim=-1) - 1).abs().max()) < 1e-4      # the padding was recomputed too


# ---- 4, 5, 6: a plane through a SIREN with one live unit per layer ------------------------------------------------------------------------
# Two networks.  "plane" is f(x) = A sin(sin(... sin(0.3 u))), u = n.x - c0, with gt_mode 'siren': df = |f| is 1-Lipschitz and its
# zero set is the plane.  But it is a SIGNED field: grad f points the same way on both sides, every sign product of the CAP-UDF rule
# is +1, and neither extractor emits a cell for it — its cell sets are equal because both are empty, and the checks on vertices hold
# over nothing.  What it does check is the call at every size, the selection on a learned-style field and the memory at 1025^3.
# "fold" is the unsigned field those checks need: the last hidden unit gets the bias pi / 60, so it is cos(2 s), s = sin(... sin(0.3 u)),
# and f = A (cos(2 s) - 1) <= 0 with A = 5 / 3; gt_mode 'tanh' with alpha = 0.3 gives df = sqrt(|f| / alpha) = |sin s| / 0.3 (|f| stays
# below 1 / alpha: A (1 - cos 1.02) = 0.80 < 3.33), which is 1-Lipschitz, zero on the plane, and whose gradient flips across it.
# A square root of a float32 difference is coarse near its zero: |f| moves in steps of A 2^-24, so df within sqrt(2^-23 A / alpha) =
# 8e-4 of the plane is noise.  The SIGNS are not (the gradient is +-n times a scalar), so the emitted cells are exactly the cells
# the plane crosses, and a vertex is at most one cell, h (|n_x| + |n_y| + |n_z|) = 1.64 h, from the plane: that is what "fold" asserts
# where "plane" has 2e-5 (interpolation error h^2 0.3 / 8 plus the value noise over the slope).
PLANE_FIELDS = {"plane": ("siren", 1.0), "fold": ("tanh", 0.3)}


def plane_model(hidden, kind="plane"):
    """First-layer row 0.01 n (w0 = 30) and bias -0.01 c0, every later layer passes unit 0 on with weight 1 / 30 (slope 1 at zero),
    everything else zero; "plane": output weight 1 / 0.3, so |grad f| <= 1.  "fold": see above."""
    from src.model import SIREN
    L, H = len(hidden), hidden[0]
    model = SIREN(3, 1, hidden, w0=30)
    sd = {}
    for i in range(L + 1):
        o, k = (H if i < L else 1), (3 if i == 0 else H)
        w = np.zeros((o, k), dtype=np.float32); b = np.zeros(o, dtype=np.float32)
        if i == 0:
            w[0] = 0.01 * PLANE_N; b[0] = -0.01 * PLANE_C0
        elif i < L:
            w[0, 0] = 1.0 / 30.0
            if kind == "fold" and i == L - 1:
                w[0, 0] = 2.0 / 30.0; b[0] = np.pi / 60.0
        else:
            w[0, 0] = 1.0 / 0.3 if kind == "plane" else 5.0 / 3.0
            if kind == "fold":
                b[0] = -w[0, 0]
        sd[f"net.{i}.0.weight"] = torch.from_numpy(w); sd[f"net.{i}.0.bias"] = torch.from_numpy(b)
    model.load_state_dict(sd)
    return model.to("cuda:0")


_plane = {}


def plane_meshes(kind, hidden, N, B):
    """(sparse fields, (v, t, cells) sparse, (v, t, cells) dense, model) for a plane network at threshold 2h; made once per case."""
    key = (kind, len(hidden), hidden[0], N, B)
    if key not in _plane:
        from diffudf_amd import hip_ops
        from src.render_mc import extract_fields, extract_fields_sparse
        model = plane_model(hidden, kind)
        mode, alpha = PLANE_FIELDS[kind]
        d = torch.device("cuda:0")
        thr = 2.0 * (2.0 / (N - 1))
        f = extract_fields_sparse(model, None, N, mode, d, alpha, threshold=thr, brick=B)
        df, vecs = extract_fields(model, None, N, mode, d, alpha)
        _plane[key] = (f, f.extract(want_cells=True), hip_ops.capudf_extract(df, vecs, threshold=thr, want_cells=True), model)
    return _plane[key]


def plane_offset(v):
    return (v * torch.tensor(PLANE_N, dtype=torch.float64, device=v.device)).sum(-1) - PLANE_C0


@pytest.mark.parametrize("kind", ["plane", "fold"])
@pytest.mark.parametrize("hidden", [[32] * 2, [256] * 8])
@pytest.mark.parametrize("N,B", [(33, 4), (33, 8), (65, 8)])
def test_end_to_end_on_a_one_lipschitz_network(kind, hidden, N, B):
    from diffudf_amd import hip_ops
    from src.render_mc import extract_mesh_CAP_sparse
    f, (v, t, c), (vd, td, cd), _ = plane_meshes(kind, hidden, N, B)
    h = 2.0 / (N - 1)
    thr = 2.0 * h
    assert f.threshold == thr and f.candidate_ids.numel() > 0 and (len(c) > 0) == (kind == "fold")
    assert cell_set(c) == cell_set(cd)
    # the sparse fields through the DENSE extractor: exactly the sparse extractor's triangles, and in the dense emission order — which
    # matches the sparse vertices with those of the dense pipeline one to one
    a, b = f.to_dense()
    vs, ts, cs = hip_ops.capudf_extract(a, b, threshold=thr, want_cells=True)
    assert np.array_equal(tri_rows(vs, ts), tri_rows(v, t))
    assert torch.equal(cs, cd) and torch.equal(ts, td) and vs.shape == vd.shape
    err = float((vs - vd).abs().max()) if len(vs) else 0.0
    print(f"{kind} {len(hidden)}x{hidden[0]} {N}/{B}: {len(c)} cells, {f.candidate_ids.numel()} candidate / {f.stored_ids.numel()} stored "
          f"bricks; max vertex difference to the dense pipeline {err:.2e}" + (" (bound 5e-5)" if kind == "plane" else ""))
    if kind == "plane":
        assert err <= 5e-5
    else:
        # the cells the plane crosses, all of them: every cell with corners on both sides, nothing else
        ax = np.linspace(-1.0, 1.0, N)
        u = np.add.outer(np.add.outer(PLANE_N[0] * ax, PLANE_N[1] * ax), PLANE_N[2] * ax) - PLANE_C0
        m = N - 1
        lo = np.full((m, m, m), np.inf); hi = -lo
        for q in range(8):
            sl = u[(q & 1):(q & 1) + m, ((q >> 1) & 1):((q >> 1) & 1) + m, ((q >> 2) & 1):((q >> 2) & 1) + m]
            lo = np.minimum(lo, sl); hi = np.maximum(hi, sl)
        assert np.abs(u).min() > 1e-6                     # no grid point on the plane: no sign is marginal
        assert cell_set(c) == {tuple(r) for r in np.argwhere((lo < 0) & (hi > 0)).tolist()}
        assert float(plane_offset(v).abs().max()) <= h * np.abs(PLANE_N).sum()
    mesh = extract_mesh_CAP_sparse(f)
    assert np.array_equal(np.asarray(mesh.vertices), v.cpu().numpy()) and np.array_equal(np.asarray(mesh.faces), t.cpu().numpy())


@pytest.mark.parametrize("kind", ["plane", "fold"])
def test_1025_cubed_stays_below_the_dense_df_array(kind):
    from src.render_mc import extract_fields_sparse
    N, B = 1025, 8
    h = 2.0 / (N - 1)
    model = plane_model([256] * 8, kind)
    mode, alpha = PLANE_FIELDS[kind]
    d = torch.device("cuda:0")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    # 2^16-point chunks: the sweeps' workspace is 16 KB per point of a chunk (8x256), 16 GB at the default 2^20 — the dense path's too
    f = extract_fields_sparse(model, None, N, mode, d, alpha, threshold=0.008, brick=B, chunk=1 << 16)
    v, t = f.extract()
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    off = float(plane_offset(v).abs().max()) if len(v) else 0.0
    print(f"1025^3 {kind}: {f.candidate_ids.numel()} candidate / {f.stored_ids.numel()} stored bricks of {S.dims(N, B)[2] ** 3}, "
          f"{f.points_stored} points ({100.0 * f.points_stored / N ** 3:.2f} % of N^3), {len(v)} vertices, {len(t)} triangles, "
          f"peak memory +{grown / 2 ** 20:.0f} MiB (dense df alone: {4 * N ** 3 / 2 ** 20:.0f} MiB), max |n.v - c0| {off:.2e}")
    assert 0 < f.points_stored < N ** 3 // 8
    assert grown < 4 * N ** 3
    assert bool(torch.isfinite(v).all())
    if kind == "plane":
        assert off <= 2e-5
    else:
        assert len(t) > 1024 ** 2                         # the plane crosses the whole cube: more than one cell per column
        assert off <= h * np.abs(PLANE_N).sum()
        assert int(t.max()) == len(v) - 1 and int(t.min()) == 0


def test_generate_mc_sparse_writes_the_mesh(tmp_path):
    import generate_mc
    from src.render_mc import extract_fields, extract_fields_sparse, extract_mesh_CAP
    hidden, N, B = [32] * 2, 33, 8
    mode, alpha = PLANE_FIELDS["fold"]
    f, (v, t, c), _, model = plane_meshes("fold", hidden, N, B)

    def read_obj(path):
        rows = [ln.split() for ln in open(path)]
        return (np.array([[float(x) for x in r[1:]] for r in rows if r[0] == "v"]),
                np.array([[int(x) for x in r[1:]] for r in rows if r[0] == "f"]) - 1)

    out = str(tmp_path / "sparse.obj")
    mesh = generate_mc.generate_mc(model, mode, 0, N, out, alpha, algorithm="cap", sparse=True, brick=B)
    assert os.path.getsize(out) > 0
    vo, to = read_obj(out)
    # generate_mc extracts at the reference's threshold 0.008, below the 2h of the shared fields: the same calls made here give the
    # same triangles bit for bit (%.17g round-trips a double), and the cells are among those of the 2h extraction
    d = torch.device("cuda:0")
    f8 = extract_fields_sparse(model, None, N, mode, d, alpha, brick=B)
    v8, t8, c8 = f8.extract(want_cells=True)
    assert f8.threshold == 0.008 and len(to) > 0 and np.array_equal(tri_rows(vo, to), tri_rows(v8, t8))
    assert np.array_equal(np.asarray(mesh.faces), to) and np.array_equal(np.asarray(mesh.vertices), vo)
    assert cell_set(c8) <= cell_set(c)
    # without the key: the dense functions' file, byte for byte
    dense = str(tmp_path / "dense.obj"); want = str(tmp_path / "want.obj")
    generate_mc.generate_mc(model, mode, 0, N, dense, alpha, algorithm="cap")
    extract_mesh_CAP(*extract_fields(model, torch.Tensor([[]]).to(d), N, mode, d, alpha), N).export(want)
    assert open(dense, "rb").read() == open(want, "rb").read()
