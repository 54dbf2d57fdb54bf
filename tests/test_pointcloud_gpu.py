# coding: utf-8
"""GPU: dense point-cloud extraction (reference src/render_pc.py:26-73) — the projection core against the reference's inner loop
(tests/golden/g14_pointcloud.npz, made by tests/golden/make_golden_pc.py), the ordered compaction against numpy boolean
indexing, and `Sampler.generate_point_cloud` end to end with both random sources."""
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HID = {"t": [128] * 4, "s": [256] * 8}


def _g14():
    return np.load(os.path.join(HERE, "golden", "g14_pointcloud.npz"))


def _model(net, G):
    from diffudf_amd import synth
    from diffudf_amd.model import SIREN
    theta = G["t_theta"] if net == "t" else synth.flatten_params(synth.siren_params(HID["s"], seed=123))
    m = SIREN(3, 1, HID[net], w0=30).cuda()
    with torch.no_grad():
        m.flat_parameters().copy_(torch.from_numpy(np.ascontiguousarray(theta)).cuda())
    return m


def _cloud_stats(p0, n0, p1, n1):
    a, b = torch.from_numpy(p0).cuda().double(), torch.from_numpy(p1).cuda().double()
    d = torch.cdist(a, b)
    d01, i01 = d.min(1); d10, i10 = d.min(0)
    n0, n1 = torch.from_numpy(n0).cuda().double(), torch.from_numpy(n1).cuda().double()
    c = 0.5 * ((n0 * n1[i01]).sum(1).abs().mean() + (n1 * n0[i10]).sum(1).abs().mean())
    return float(0.5 * (d01.mean() + d10.mean())), float(c)


@pytest.mark.parametrize("net", ["t", "s"])
@pytest.mark.parametrize("mode", ["tanh", "siren"])
def test_project_points_against_reference_inner_loop(net, mode):
    """Accept flags equal the reference's on >= 99 % of the points (the allowance tests/test_api_gpu.py grants rays at a
    threshold; the reference's own float32 / float64 runs agree on >= 99.5 %, `*_fate`); where they agree, moved positions
    within 1e-4 and |n.n_ref| >= 1 - 1e-3 for the points whose top two Hessian eigenvalues are separated by more than 1e-2 of
    the largest.  Points with udf < 0 under 'tanh' are rejected and NaN.
    Measured (MI355X): every fate equal in all four cases; max |moved - ref| 4.7e-5 (4x128 trained) / 2.3e-5 (8x256);
    min |n.n_ref| 0.999999; no accepted point left out by the eigenvalue-separation rule."""
    from diffudf_amd import hip_ops
    G = _g14()
    m = _model(net, G)
    cfg, theta = m.hip_cfg, m.flat_parameters()
    k = f"{net}_{mode}_"
    pts = torch.from_numpy(G[f"{net}_start"].copy()).cuda()
    last, unit, pre, acc = hip_ops.project_points(cfg, theta, pts, mode, float(G["alpha"]), int(G["num_steps"]),
                                                  float(G["surf_thresh"]))
    moved, acc, last = pts.cpu().numpy(), acc.cpu().numpy().astype(bool), last.cpu().numpy()
    ref_acc, ref_moved = G[k + "accept"].astype(bool), G[k + "moved"]
    same = acc == ref_acc
    print(f"{net}/{mode}: accepted {acc.sum()} (reference {ref_acc.sum()}), same fate {same.mean():.4f}")
    assert same.mean() >= 0.99
    nan_ref = np.isnan(ref_moved).any(1)
    assert np.array_equal(np.isnan(moved).any(1) & same, nan_ref & same) and not acc[np.isnan(moved).any(1)].any()
    if mode == "tanh":
        neg = G[k + "udf"] < 0                      # last-step udf < 0: NaN step there, NaN point here, rejected
        assert not acc[neg & same].any() and np.isnan(last[neg & same]).all()
    ok = same & ~nan_ref
    err = np.abs(moved[ok] - ref_moved[ok]).max()
    print(f"  moved positions: max |diff| {err:.2e} over {ok.sum()} points")
    assert err < 1e-4
    both = acc & ref_acc
    if mode == "siren":
        nrm = unit.cpu().numpy()
        keep = both
    else:
        _, _, _, _, V = hip_ops.query_frame(cfg, theta, pre)
        nrm = V[:, :, 2].cpu().numpy().astype(np.float64)
        H = G[k + "hess"].astype(np.float64)
        lam = np.full((len(H), 3), np.nan)
        fin = np.isfinite(H).all(axis=(1, 2))
        lam[fin] = np.linalg.eigvalsh(H[fin])
        with np.errstate(invalid="ignore"):
            keep = both & ((lam[:, 2] - lam[:, 1]) > 1e-2 * np.abs(lam).max(1))
        left_out = 1 - keep.sum() / max(both.sum(), 1)
        print(f"  normals: {both.sum() - keep.sum()} of {both.sum()} accepted points left out (near-degenerate top eigenvalues)")
        if net == "t":
            assert left_out < 0.05
    if keep.any():
        dots = np.abs((nrm[keep] * G[k + "normals"][keep].astype(np.float64)).sum(1))
        print(f"  normals: min |n.n_ref| {dots.min():.6f} over {keep.sum()} points")
        assert dots.min() >= 1 - 1e-3


@pytest.mark.parametrize("case", ["none", "all", "one", "odd", "million"])
def test_compaction_is_numpy_boolean_indexing(case):
    from diffudf_amd import hip_ops
    rng = np.random.default_rng(11)
    n = {"none": 1000, "all": 1000, "one": 1, "odd": 64 * 7 + 13, "million": 1000003}[case]
    mask = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "one": np.ones(n, bool)}.get(case)
    if mask is None:
        mask = rng.random(n) < 0.37
    a, b, f = rng.normal(size=(n, 3)), rng.normal(size=(n, 3)), rng.normal(size=(n, 3)).astype(np.float32)
    cap = 2 * n + 5
    d = lambda x: torch.from_numpy(x).cuda()  # noqa: E731
    dst_a = torch.full((cap, 3), -7.0, dtype=torch.float64, device="cuda"); dst_b = dst_a.clone()
    out_f = torch.full((n, 3), -7.0, dtype=torch.float32, device="cuda")
    counter = torch.zeros(4, dtype=torch.int64, device="cuda")
    flags = d(mask.astype(np.uint8))
    hip_ops.pointcloud_append(flags, d(a), dst_a, counter, src_b=d(b), dst_b=dst_b, src_f=d(f), out_f=out_f)
    k = int(mask.sum())
    assert counter.tolist()[:3] == [k, k, 0]
    assert np.array_equal(dst_a[:k].cpu().numpy(), a[mask]) and np.array_equal(dst_b[:k].cpu().numpy(), b[mask])
    assert np.array_equal(out_f[:k].cpu().numpy(), f[mask])
    assert bool((dst_a[k:] == -7.0).all()) and bool((out_f[k:] == -7.0).all())
    # a second append continues at the counter, in order
    mask2 = ~mask if case != "none" else np.ones(n, bool)
    hip_ops.pointcloud_append(d(mask2.astype(np.uint8)), d(b), dst_a, counter)
    k2 = int(mask2.sum())
    assert counter.tolist()[:3] == [k + k2, k2, k]
    assert np.array_equal(dst_a[:k + k2].cpu().numpy(), np.vstack((a[mask], b[mask2])))
    # quota reached / no room: nothing is added
    hip_ops.pointcloud_append(flags, d(a), dst_a, counter, quota=1)
    assert counter.tolist()[:3] == [k + k2, 0, k + k2]
    if k >= 2:
        small = torch.zeros(k - 1, 3, dtype=torch.float64, device="cuda")
        c2 = torch.zeros(4, dtype=torch.int64, device="cuda")
        hip_ops.pointcloud_append(flags, d(a), small, c2)
        assert c2.tolist()[:2] == [0, 0] and bool((small == 0).all())


def test_generate_point_cloud_numpy_stream():
    """rng="numpy", np.random.seed(0): round 0 proposals are bit-equal to the reference's first draw; >= num_points rows, all in
    the domain and near the zero set when re-queried; against the fixture's seed-0 cloud of the reference's own Sampler the
    symmetric mean nearest-neighbour distance is <= 2 d_ref and the normal agreement >= c_ref - 0.05 (two independent samplings
    of one surface differ by about d_ref).
    Measured (MI355X): 4892 rows, the reference's count for this seed; distance to its cloud 0.00000 (d_ref 0.00571), normal
    agreement 1.0000 (c_ref 0.9989) — the same stream gives the same cloud.  rng="device" (next test): 4964 rows, 0.00564, 0.9989."""
    from diffudf_amd import hip_ops
    from src.render_pc import Sampler
    G = _g14()
    m = _model("t", G)
    cfg, theta = m.hip_cfg, m.flat_parameters()
    np.random.seed(0)
    st = hip_ops.PointCloudState(cfg, 4096, "cuda:0")
    buf = np.random.uniform(-1, 1, (4096, 3))
    hip_ops.pointcloud_round(cfg, theta, st, "tanh", float(G["alpha"]), rand=torch.from_numpy(buf.reshape(-1)).cuda())
    assert np.array_equal(st.proposals().cpu().numpy(), buf)          # the reference's first draw (:39), bit for bit
    np.random.seed(0)
    s = Sampler.from_model(m)
    p, nrm = s.generate_point_cloud("tanh", float(G["alpha"]), int(G["num_steps"]), 4096, float(G["surf_thresh"]), 200)
    assert p.dtype == np.float64 and nrm.dtype == np.float64 and p.shape == nrm.shape and p.shape[0] >= 4096 and p.shape[1] == 3
    assert (np.abs(p) <= 1).all() and np.isfinite(nrm).all()
    f, _ = hip_ops.query(cfg, theta, torch.from_numpy(p).cuda().float())
    assert torch.isfinite(f).all()
    assert np.allclose(np.linalg.norm(nrm, axis=1), 1.0, atol=1e-5)
    dist, c = _cloud_stats(p, nrm, G["e2e_points0"].astype(np.float64), G["e2e_normals0"].astype(np.float64))
    print(f"numpy stream: {len(p)} rows, d {dist:.5f} (d_ref {float(G['e2e_d_ref']):.5f}), c {c:.4f} (c_ref {float(G['e2e_c_ref']):.4f})")
    assert dist <= 2 * float(G["e2e_d_ref"]) and c >= float(G["e2e_c_ref"]) - 0.05


def test_generate_point_cloud_device_rng():
    from src.render_pc import Sampler
    G = _g14()
    m = _model("t", G)
    s = Sampler.from_model(m)
    kw = dict(gt_mode="tanh", alpha=float(G["alpha"]), num_steps=int(G["num_steps"]), num_points=4096,
              surf_thresh=float(G["surf_thresh"]), max_iter=200, rng="device")
    p0, n0 = s.generate_point_cloud(seed=5, **kw)
    p1, n1 = s.generate_point_cloud(seed=5, check_every=3, **kw)
    p2, _ = s.generate_point_cloud(seed=6, **kw)
    assert np.array_equal(p0, p1) and np.array_equal(n0, n1) and len(p0) >= 4096
    assert p2.shape != p0.shape or not np.array_equal(p0, p2)
    dist, c = _cloud_stats(p0, n0, G["e2e_points0"].astype(np.float64), G["e2e_normals0"].astype(np.float64))
    print(f"device rng: {len(p0)} rows, d {dist:.5f}, c {c:.4f}")
    assert dist <= 2 * float(G["e2e_d_ref"]) and c >= float(G["e2e_c_ref"]) - 0.05
    # 'siren' rounds only enqueue between count checks: the result does not depend on check_every
    q0, m0 = s.generate_point_cloud("siren", 1.0, 5, 2000, 0.01, 64, rng="device", seed=9, check_every=1)
    q1, m1 = s.generate_point_cloud("siren", 1.0, 5, 2000, 0.01, 64, rng="device", seed=9, check_every=8)
    assert np.array_equal(q0, q1) and np.array_equal(m0, m1)
    t0, t1 = s.generate_point_cloud("tanh", 100.0, 5, 512, 0.01, 50, rng="device", seed=3, return_tensors=True)
    assert t0.is_cuda and t0.dtype == torch.float64 and t0.shape == t1.shape


def test_empty_field_reaches_max_iter():
    """A bias-shifted network (f >= 1 everywhere in the box): nothing is ever accepted — RuntimeWarning and two (0,3) arrays."""
    from src.render_pc import Sampler
    G = _g14()
    m = _model("t", G)
    with torch.no_grad():
        m.net[-1][0].bias += 5.0
    s = Sampler.from_model(m)
    for rng in ("numpy", "device"):
        with pytest.warns(RuntimeWarning, match="Max iterations reached"):
            p, n = s.generate_point_cloud("tanh", 100.0, num_points=1000, max_iter=3, rng=rng, seed=1)
        assert p.shape == (0, 3) and n.shape == (0, 3) and p.dtype == np.float64


@pytest.mark.parametrize("num_points", [0, 1, 777])
@pytest.mark.parametrize("mode", ["tanh", "siren"])
def test_edge_sizes(num_points, mode):
    from diffudf_amd import hip_ops
    from src.render_pc import Sampler
    G = _g14()
    m = _model("t", G)
    s = Sampler.from_model(m)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for rng in ("numpy", "device"):
            p, n = s.generate_point_cloud(mode, 100.0, num_points=num_points, max_iter=30, rng=rng, seed=2)
            assert p.shape == n.shape and p.ndim == 2 and p.shape[1] == 3 and p.dtype == np.float64
            if num_points == 777:
                assert len(p) >= 777
            if num_points == 0:
                assert len(p) == 0
    empty = torch.zeros(0, 3, dtype=torch.float64, device="cuda")
    last, unit, pre, acc = hip_ops.project_points(m.hip_cfg, m.flat_parameters(), empty, mode, 100.0)
    assert last.shape == (0,) and unit.shape == (0, 3) and pre.shape == (0, 3) and acc.shape == (0,)
