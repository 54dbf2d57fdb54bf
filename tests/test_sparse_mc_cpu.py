# coding: utf-8
"""CPU: the brick-sparse narrow band without a GPU — the numpy oracle of the selection and what it guarantees
(the candidate bricks cover every active cell of the analytic fields, which is what lets the GPU comparisons ask for equality),
gather / scatter, the host arithmetic of the C ABI (sizes, every refusal, returned before any launch) and the Python refusals."""
import ctypes

import numpy as np
import pytest

import sparsegrid_oracle as S
from test_capudf import analytic_fields
from diffudf_amd import _lib

OK, E_CFG, E_WS, E_MODE, E_UNSUP = 0, -1, -2, -3, -4

_arena = ctypes.create_string_buffer(1 << 22)
BASE = (ctypes.addressof(_arena) + 255) // 256 * 256    # 256-byte aligned; stands in for any device pointer (never read)
P = ctypes.c_void_p(BASE)

# (kind, N, B, threshold in voxels or None = 0.008, lipschitz) -> candidate bricks the rule gives (of nb^3).  Two of them are the
# figures of the numpy model the rule was proposed with (sheet 129 / 8 / 0.008 / 1.25: 608 of 4096; sheet 33 / 4: 200 of 512).
CANDIDATES = {
    ("sphere", 20, 8): (27, 27, 27, 27), ("sphere", 33, 8): (64, 64, 64, 64), ("sphere", 65, 8): (238, 292, 292, 324),
    ("sphere", 33, 4): (238, 292, 329, 389), ("sphere", 129, 8): (870, 973, 957, 1087),
    ("sheet", 20, 8): (27, 27, 27, 27), ("sheet", 33, 8): (48, 56, 56, 64), ("sheet", 65, 8): (164, 200, 200, 224),
    ("sheet", 33, 4): (164, 200, 224, 280), ("sheet", 129, 8): (484, 608, 592, 688),
}                                                       # order: (0.008, 1.0), (0.008, 1.25), (2h, 1.0), (2h, 1.25)


def coarse_of(ndf, N, B):
    ix = S.lattice_indices(N, B)
    return ndf[np.ix_(ix, ix, ix)]


@pytest.mark.parametrize("kind,N,B", sorted(CANDIDATES))
def test_candidate_bricks_cover_every_active_cell(kind, N, B):
    ndf, _ = analytic_fields(N, kind)
    coarse = coarse_of(ndf, N, B)
    m, nb, nl = S.dims(N, B)
    counts = []
    for thr in (0.008, 2.0 * (2.0 / (N - 1))):
        active = S.active_cells(ndf, thr)
        assert active.any()
        for lip in (1.0, 1.25):
            slot, stored, cand = S.select(coarse, N, B, S.bound(N, B, thr, lip))
            assert not (active & ~S.candidate_cell_mask(cand, N, B)).any(), (thr, lip)
            counts.append(len(cand))
            # the structure: ascending lists, slots in list order, candidates stored, every corner of a candidate's cells stored
            assert np.all(np.diff(stored) > 0) and np.all(np.diff(cand) > 0)
            assert np.array_equal(slot.reshape(-1)[stored], np.arange(len(stored))) and (slot >= 0).sum() == len(stored)
            c = np.stack([cand // (nl * nl), (cand // nl) % nl, cand % nl], -1)
            assert (c < nb).all()
            for d in range(8):
                q = np.minimum(c + np.array([d & 1, (d >> 1) & 1, (d >> 2) & 1]), nl - 1)
                assert (slot[q[:, 0], q[:, 1], q[:, 2]] >= 0).all()
    assert tuple(counts) == CANDIDATES[(kind, N, B)]


def test_lattice_and_dims():
    assert S.dims(2, 4) == (1, 1, 1) and S.dims(5, 4) == (4, 1, 2) and S.dims(9, 8) == (8, 1, 2)
    assert S.dims(20, 8) == (19, 3, 3) and S.dims(33, 4) == (32, 8, 9) and S.dims(1025, 8) == (1024, 128, 129)
    assert S.lattice_indices(20, 8).tolist() == [0, 8, 16, 19] and S.lattice_indices(9, 8).tolist() == [0, 8]
    assert S.lattice_indices(2, 4).tolist() == [0, 1]
    from diffudf_amd import hip_ops
    for N, B in ((2, 4), (5, 4), (20, 8), (33, 4), (1025, 8)):
        assert hip_ops.sparse_dims(N, B) == S.dims(N, B)
        assert hip_ops.sparse_bound(N, B, 0.008, 1.25) == S.bound(N, B, 0.008, 1.25)


def test_nan_and_equality_in_the_selection():
    """A NaN corner makes its bricks candidates; a corner exactly equal to the bound selects (<=), the next float above does not."""
    N, B = 33, 8
    m, nb, nl = S.dims(N, B)
    bnd = 0.25                                           # exactly representable in float32
    coarse = np.full((nb + 1,) * 3, 1.0, dtype=np.float32)
    coarse[0, 0, 0] = np.float32(bnd)
    coarse[4, 4, 4] = np.nan
    coarse[2, 0, 4] = np.nextafter(np.float32(bnd), np.float32(1))
    slot, stored, cand = S.select(coarse, N, B, bnd)
    ids = lambda *b: [(x * nl + y) * nl + z for x, y, z in b]     # noqa: E731
    assert cand.tolist() == sorted(ids((0, 0, 0), (3, 3, 3)))       # the NaN at lattice point 4 touches cell brick 3 only (nb = 4)
    assert stored.tolist() == sorted(ids(*[(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)],
                                         *[(x, y, z) for x in (3, 4) for y in (3, 4) for z in (3, 4)]))


@pytest.mark.parametrize("N,B", [(20, 8), (13, 4), (9, 8), (2, 4)])
def test_gather_scatter_round_trip(N, B):
    ndf, vec = analytic_fields(N, "sheet")
    slot, stored, cand = S.select(coarse_of(ndf, N, B), N, B, 1e9)          # everything stored
    assert len(stored) == S.dims(N, B)[2] ** 3
    df, v = S.gather(ndf, vec, stored, N, B)
    assert df.shape == (len(stored), B, B, B) and v.shape == df.shape + (3,)
    a, b = S.scatter(df, v, stored, N, B)
    assert np.array_equal(a, ndf) and np.array_equal(b, vec)
    slot, stored, cand = S.select(coarse_of(ndf, N, B), N, B, S.bound(N, B, 0.008, 1.25))
    a, b = S.scatter(*S.gather(ndf, vec, stored, N, B), stored, N, B)
    keep = ~np.isnan(a)
    assert np.array_equal(a[keep], ndf[keep]) and keep.sum() == S.brick_points(stored, N, B)[1].sum()


def test_sizes_of_the_c_abi():
    L = _lib.load()
    r = lambda b: (b + 255) // 256 * 256                 # noqa: E731
    for N, B in ((2, 4), (33, 8), (65, 8), (1025, 8), (2049, 8), (33, 4)):
        m, nb, nl = S.dims(N, B)
        blocks = (nl ** 3 + 255) // 256
        assert L.dudf_sparse_select_bytes(N, B) == r(blocks * 16) + r(blocks * 8) + r(nl ** 3)
        for nc in (0, 1, min(nb ** 3, (2 ** 31 - 1) // B ** 3)):      # all cell bricks, or as many as 2^31 - 1 cells allow
            cb = (nc * B ** 3 + 255) // 256
            assert L.dudf_capudf_sparse_workspace_bytes(N, B, nc) == r(max(cb, 1) * 24) + r(max(cb, 1) * 12)
    # refusals answer 0: a brick edge other than 4 or 8, N < 2, more candidates than cell bricks, a lattice beyond 2^31 - 1 entries
    assert L.dudf_sparse_select_bytes(33, 5) == 0 and L.dudf_sparse_select_bytes(1, 8) == 0
    assert L.dudf_sparse_select_bytes(10313, 8) > 0 and L.dudf_sparse_select_bytes(10314, 8) == 0
    assert L.dudf_sparse_select_bytes(5157, 4) > 0 and L.dudf_sparse_select_bytes(5158, 4) == 0
    assert L.dudf_capudf_sparse_workspace_bytes(33, 8, 65) == 0 and L.dudf_capudf_sparse_workspace_bytes(33, 8, -1) == 0
    assert L.dudf_capudf_sparse_workspace_bytes(33, 16, 1) == 0


def test_refusals_return_before_any_launch():
    """As tests/test_cabi_errors.py: the "device" pointers are a host address that a refused call never reads, so every code below is
    returned before the first HIP call (this process has no GPU)."""
    L = _lib.load()
    cfg = ctypes.byref(_lib.NetCfg(3, 2, 32, 30.0))
    nq = L.dudf_workspace_bytes_query(cfg, 512, 0)
    lattice = lambda N=33, B=8, start=0, count=8, mode=0, df=P, ws=P, nb=nq, c=cfg: L.dudf_grid_fields_lattice(   # noqa: E731
        c, P, N, B, start, count, mode, 1.0, df, None, None, ws, nb, None)
    assert lattice(B=5) == E_CFG and lattice(B=16) == E_CFG and lattice(N=1) == E_CFG and lattice(df=None) == E_CFG
    assert lattice(start=-1) == E_CFG and lattice(start=120, count=6) == E_CFG           # 5^3 = 125 lattice points
    assert lattice(mode=3) == E_MODE and lattice(mode=-1) == E_MODE
    assert lattice(N=10314) == E_UNSUP and lattice(N=5158, B=4) == E_UNSUP
    assert lattice(N=65, nb=nq - 1, count=512) == E_WS and lattice(ws=None) == E_WS and lattice(c=None) == E_CFG
    assert lattice(count=0) == OK

    ns = L.dudf_sparse_select_bytes(33, 8)
    select = lambda N=33, B=8, a=(P, P, P, P, P), ws=P, nb=ns: L.dudf_sparse_select(a[0], N, B, 0.1, a[1], a[2], a[3], a[4], ws, nb, None)  # noqa: E731
    assert select(B=2) == E_CFG and select(N=0) == E_CFG and select(N=10314) == E_UNSUP
    for k in range(5):
        assert select(a=tuple(None if i == k else P for i in range(5))) == E_CFG
    assert select(nb=ns - 1) == E_WS and select(ws=None) == E_WS and select(ws=ctypes.c_void_p(BASE + 8)) == E_WS

    nq = L.dudf_workspace_bytes_query(cfg, 2 * 512, 0)
    bricks = lambda N=33, B=8, n=2, mode=1, a=(P, P, P), ws=P, nb=nq: L.dudf_grid_fields_bricks(   # noqa: E731
        cfg, P, N, B, a[0], n, mode, 1.0, a[1], a[2], P, ws, nb, None)
    assert bricks(B=7) == E_CFG and bricks(N=1) == E_CFG and bricks(n=-1) == E_CFG and bricks(n=126) == E_CFG   # nl^3 = 125
    for k in range(3):
        assert bricks(a=tuple(None if i == k else P for i in range(3))) == E_CFG
    assert bricks(mode=5) == E_MODE and bricks(N=10314) == E_UNSUP
    assert bricks(N=10313, n=(1 << 22)) == E_UNSUP                                         # 2^22 bricks of 512 points = 2^31
    assert bricks(nb=nq - 1) == E_WS and bricks(n=0) == OK

    nc = L.dudf_capudf_sparse_workspace_bytes(33, 8, 3)
    head = lambda a, n, N, B: (a[0], a[1], a[2], a[3], n, N, B, 0.008)                  # noqa: E731
    count = lambda N=33, B=8, n=3, a=(P, P, P, P), out=P, ws=P, nb=nc: L.dudf_capudf_sparse_count(*head(a, n, N, B), out, ws, nb, None)  # noqa: E731
    emit = lambda N=33, B=8, n=3, a=(P, P, P, P), v=P, t=P, ws=P, nb=nc: L.dudf_capudf_sparse_emit(*head(a, n, N, B), v, t, None, ws, nb, None)  # noqa: E731
    for call in (count, emit):
        assert call(B=3) == E_CFG and call(N=1) == E_CFG and call(n=-1) == E_CFG and call(n=65) == E_CFG
        assert call(N=10314) == E_UNSUP and call(N=10313, n=1 << 22) == E_UNSUP
        for k in range(4):
            assert call(a=tuple(None if i == k else P for i in range(4))) == E_CFG
        assert call(nb=nc - 1) == E_WS and call(ws=None) == E_WS
    assert count(out=None) == E_CFG and emit(v=None) == E_CFG and emit(t=None) == E_CFG


def test_python_refusals():
    import torch
    import generate_mc
    from diffudf_amd import hip_ops
    from src.render_mc import SparseFields, extract_fields_sparse, extract_mesh_CAP_sparse
    with pytest.raises(_lib.DudfError, match="'cap' only"):
        generate_mc.generate_mc(None, "tanh", "cpu", 33, "unused.obj", 100, algorithm="both", sparse=True)
    for alg in ("meshudf", "siren"):
        with pytest.raises(_lib.DudfError):
            generate_mc.generate_mc(None, "tanh", "cpu", 33, "unused.obj", 100, algorithm=alg, sparse=True)
    ndf, vec = analytic_fields(20, "sheet")
    with pytest.raises(_lib.DudfError, match="CUDA tensor"):
        SparseFields.from_dense(torch.from_numpy(ndf), torch.from_numpy(vec))
    with pytest.raises(_lib.DudfError, match="CUDA tensor"):
        hip_ops.sparse_select(torch.zeros(64), 20, 8, 0.1)
    with pytest.raises(_lib.DudfError):
        hip_ops.sparse_dims(20, 5)
    with pytest.raises(_lib.DudfError, match="needs the GPU"):
        extract_fields_sparse(None, None, 33, "tanh", "cpu", 100)
    f = SparseFields(20, 8, 0.008, 1.25, None, None, None, None, None)
    with pytest.raises(ValueError, match="exceeds"):
        extract_mesh_CAP_sparse(f, threshold=0.01)
    assert "lipschitz" in extract_fields_sparse.__doc__ and "statement about their field" in extract_fields_sparse.__doc__
