# coding: utf-8
"""GPU: Chamfer distance / normal consistency (diffudf_amd/metrics.py, csrc/dudf_chamfer.hip, cuantitative.py) against the float64
oracle of tests/chamfer_oracle.py (pinned by tests/test_chamfer_cpu.py), on 100 000 x 60 000 points sampled from the beetle.

Tolerances (u = 2^-24, the unit round-off of fp32):
  distances   |d - d_min| <= 8 u d_min for EVERY row: each difference is one rounding; square or abs plus the three-term sum add at
              most four more, so the fp32 distance of any candidate is within 5u of its true value and the winner's within 5u of the
              true minimum; 8u leaves room for contraction choices;
  indices     in range; the float64 distance to the chosen row within 16u of the float64 minimum; equal to the oracle's index wherever
              the float64 runner-up is more than (1 + 1e-5) times the nearest (>= 99.9 % of the rows must be of that kind);
  cham_dist   1e-6 relative (about twice the per-term bound plus the final fp32 rounding);
  cham_normals 2e-6 absolute, the oracle's normal term evaluated at the device's (validated) indices;
  normals     1e-6 per component against the float64 `np.add.at` restatement."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chamfer_oracle as CO  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -24
DEV = "cuda:0"


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def beetle():
    from diffudf_amd import mesh
    v, t = mesh.load_obj(os.path.join(HERE, "golden", "beetle.obj"))
    return mesh.normalize_vertices(v), t


@pytest.fixture(scope="module")
def clouds(beetle):
    from diffudf_amd import mesh
    v, t = beetle
    x, xn = mesh.sample_surface(v, t, 100000, seed=1)
    y, yn = mesh.sample_surface(v, t, 60000, seed=2)
    return x, xn, y, yn


@pytest.fixture(scope="module")
def oracle_nn(clouds):
    """{(direction, norm): (d1, i1, d2)} in float64 on the same float32 inputs."""
    x, _, y, _ = clouds
    out = {}
    for norm in (1, 2):
        out["xy", norm] = CO.nearest(x, y, norm, device=DEV)
        out["yx", norm] = CO.nearest(y, x, norm, device=DEV)
    return out


def _check_nearest(p, q, norm, dist, idx, oracle):
    """The per-point and index bounds of the module docstring; returns the figures it asserted on."""
    d1, i1, d2 = oracle
    m = len(q)
    assert dist.dtype == np.float32 and idx.dtype == np.int64 and dist.shape == idx.shape == (len(p),)
    err = np.abs(dist.astype(np.float64) - d1)
    worst = float((err / np.maximum(d1, 1e-300)).max())
    print(f"norm {norm}: max |d - d_min| / d_min = {worst / U:.3f} u over {len(p)} rows")
    assert (err <= 8 * U * d1).all(), worst / U
    assert idx.min() >= 0 and idx.max() < m
    at = CO.pair_distance(p, q[idx], norm)
    rel = float(((at - d1) / np.maximum(d1, 1e-300)).max())
    print(f"norm {norm}: float64 distance at the returned index exceeds the minimum by at most {rel / U:.3f} u")
    assert (at - d1 <= 16 * U * d1).all(), rel / U
    clear = d2 > (1.0 + 1e-5) * d1
    share = float(clear.mean())
    print(f"norm {norm}: rows with a clear winner {share:.6f}; index mismatches among them {int((idx[clear] != i1[clear]).sum())}")
    assert share >= 0.999
    assert np.array_equal(idx[clear], i1[clear])
    return worst, rel, share


@pytest.mark.parametrize("norm", [1, 2])
def test_nearest_points_against_the_oracle(clouds, oracle_nn, norm):
    from diffudf_amd import metrics
    x, _, y, _ = clouds
    for tag, p, q in (("xy", x, y), ("yx", y, x)):
        dist, idx = metrics.nearest_points(_cuda(p), _cuda(q), norm)
        _check_nearest(p, q, norm, dist.cpu().numpy(), idx.cpu().numpy(), oracle_nn[tag, norm])
    # identical points: exactly 0, and the point itself unless an earlier row coincides with it
    dist, idx = metrics.nearest_points(_cuda(x), _cuda(x), norm)
    assert (dist == 0).all() and (idx <= torch.arange(len(x), device=DEV)).all()
    assert np.array_equal(x[idx.cpu().numpy()], x)


@pytest.mark.parametrize("norm", [1, 2])
def test_tie_rule_and_order_independence(clouds, norm):
    from diffudf_amd import hip_ops, metrics
    x, xn, y, yn = clouds
    xd, yd = _cuda(x), _cuda(y)
    d0, i0 = metrics.nearest_points(xd, yd, norm)
    # y' = concat(y, y): another launch geometry, every distance tied at least twice — the smaller index wins, same bits
    d2, i2 = metrics.nearest_points(xd, torch.cat([yd, yd]), norm)
    assert int(i2.max()) < len(y) and torch.equal(i2, i0)
    assert torch.equal(d2.view(torch.int32), d0.view(torch.int32))
    # permuting the rows of x permutes the outputs
    perm = torch.from_numpy(np.random.default_rng(5).permutation(len(x))).to(DEV)
    dp, ip = metrics.nearest_points(xd[perm].contiguous(), yd, norm)
    assert torch.equal(dp.view(torch.int32), d0[perm].view(torch.int32)) and torch.equal(ip, i0[perm])
    # two calls are bit-identical, distances, indices and the sums behind the means
    d1, i1 = metrics.nearest_points(xd, yd, norm)
    assert torch.equal(d1.view(torch.int32), d0.view(torch.int32)) and torch.equal(i1, i0)
    s0 = hip_ops.chamfer_terms(d0, i0, _cuda(xn), _cuda(yn))
    s1 = hip_ops.chamfer_terms(d1, i1, _cuda(xn), _cuda(yn))
    assert torch.equal(s0.view(torch.int64), s1.view(torch.int64)) and torch.isfinite(s0).all()
    # the sums themselves: double accumulation of the fp32 distances / of the oracle's normal term at these indices.  Both sides
    # are float64: a term is off by a few 2^-53 (absolute, it is at most 1) and so is each of the 1e5 additions relative to the
    # running sum, about 1e-11 of the sum in all; 1e-9 leaves two digits
    want_d = d0.cpu().numpy().astype(np.float64).sum()
    want_n = CO.normal_term(xn, yn, i0.cpu().numpy()).sum()
    assert abs(float(s0[0]) - want_d) <= 1e-12 * want_d and abs(float(s0[1]) - want_n) <= 1e-9 * max(want_n, 1.0)
    only = hip_ops.chamfer_terms(d0, None)
    assert float(only[0]) == float(s0[0]) and float(only[1]) == 0.0


@pytest.mark.parametrize("norm", [1, 2])
def test_sizes_off_every_tile(norm):
    """n, m in {1, 63, 65, 1000, 4097}: not multiples of the rows per lane, per workgroup or per LDS tile; m below one y tile."""
    from diffudf_amd import metrics
    rng = np.random.default_rng(11)
    pts = rng.uniform(-1, 1, (4097, 3)).astype(np.float32)
    qts = rng.uniform(-1, 1, (4097, 3)).astype(np.float32)
    for n in (1, 63, 65, 1000, 4097):
        for m in (1, 63, 65, 1000, 4097):
            p, q = pts[:n], qts[:m]
            dist, idx = metrics.nearest_points(_cuda(p), _cuda(q), norm)
            dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
            d1, i1, d2 = CO.nearest(p, q, norm, device=DEV)
            assert idx.min() >= 0 and idx.max() < m, (n, m)
            assert (np.abs(dist - d1) <= 8 * U * d1).all(), (n, m)
            assert (CO.pair_distance(p, q[idx], norm) - d1 <= 16 * U * d1).all(), (n, m)
            clear = d2 > (1.0 + 1e-5) * d1
            assert np.array_equal(idx[clear], i1[clear]), (n, m)
    d, i = metrics.nearest_points(torch.zeros(0, 3, device=DEV), _cuda(qts), norm)
    assert d.shape == (0,) and i.shape == (0,)


@pytest.mark.parametrize("norm", [1, 2])
def test_nan_row_and_argument_errors(norm):
    from diffudf_amd import _lib, hip_ops, metrics
    rng = np.random.default_rng(13)
    p = rng.uniform(-1, 1, (3000, 3)).astype(np.float32); q = rng.uniform(-1, 1, (5000, 3)).astype(np.float32)
    d0, i0 = metrics.nearest_points(_cuda(p), _cuda(q), norm)
    bad = p.copy(); bad[17, 1] = np.nan; bad[2999, 0] = np.nan
    d, i = metrics.nearest_points(_cuda(bad), _cuda(q), norm)
    assert torch.isnan(d[17]) and torch.isnan(d[2999]) and 0 <= int(i[17]) < 5000 and 0 <= int(i[2999]) < 5000
    keep = torch.ones(3000, dtype=torch.bool, device=DEV); keep[17] = False; keep[2999] = False
    assert torch.equal(d[keep].view(torch.int32), d0[keep].view(torch.int32)) and torch.equal(i[keep], i0[keep])
    with pytest.raises(_lib.DudfError, match="BADMODE"):
        hip_ops.nearest_points(_cuda(p), _cuda(q), 3)
    with pytest.raises(_lib.DudfError, match="BADCFG"):
        hip_ops.nearest_points(_cuda(p), torch.zeros(0, 3, device=DEV), norm)
    # a misaligned / short workspace is refused before anything is launched
    lib = _lib.load()
    xd, yd = _cuda(p), _cuda(q)
    ws = torch.empty(int(lib.dudf_nearest_workspace_bytes(3000)) + 256, dtype=torch.uint8, device=DEV)
    V = ctypes.c_void_p
    args = (V(xd.data_ptr()), 3000, V(yd.data_ptr()), 5000, norm, V(0), V(0))
    assert lib.dudf_nearest_points(*args, V(ws.data_ptr() + 8), ws.numel() - 8, V(0)) == -2
    assert lib.dudf_nearest_points(*args, V(ws.data_ptr()), 1024, V(0)) == -2


@pytest.mark.parametrize("norm", [1, 2])
def test_chamfer_distance_against_the_oracle(clouds, oracle_nn, norm):
    from diffudf_amd import metrics
    x, xn, y, yn = clouds
    xd, yd, xnd, ynd = _cuda(x), _cuda(y), _cuda(xn), _cuda(yn)
    (dxy, _, _), (dyx, _, _) = oracle_nn["xy", norm], oracle_nn["yx", norm]
    want_cd = dxy.mean() + dyx.mean()
    ixy = metrics.nearest_points(xd, yd, norm)[1].cpu().numpy()            # validated by test_nearest_points_against_the_oracle
    iyx = metrics.nearest_points(yd, xd, norm)[1].cpu().numpy()
    want_nc = CO.normal_term(xn, yn, ixy).mean() + CO.normal_term(yn, xn, iyx).mean()
    cd, nc = metrics.chamfer_distance(xd, yd, norm=norm)
    assert nc is None and cd.dtype == torch.float32 and cd.dim() == 0 and cd.is_cuda
    print(f"norm {norm}: cham_dist {float(cd):.9e} oracle {want_cd:.9e} rel {abs(float(cd) - want_cd) / want_cd:.2e}")
    assert abs(float(cd) - want_cd) <= 1e-6 * want_cd
    cd2, nc2 = metrics.chamfer_distance(xd, yd, xnd, ynd, norm=norm)
    print(f"norm {norm}: cham_normals {float(nc2):.9e} oracle {want_nc:.9e} abs {abs(float(nc2) - want_nc):.2e}")
    assert float(cd2) == float(cd) and nc2.dtype == torch.float32 and nc2.dim() == 0
    assert abs(float(nc2) - want_nc) <= 2e-6
    # (2, P, 3): second batch element = the clouds of the other direction cut to the same lengths
    P1, P2 = 50000, 40000
    xb = torch.stack([xd[:P1], yd[:P1]]); yb = torch.stack([yd[:P2], xd[P1:P1 + P2]])
    xnb = torch.stack([xnd[:P1], ynd[:P1]]); ynb = torch.stack([ynd[:P2], xnd[P1:P1 + P2]])
    cdb, ncb = metrics.chamfer_distance(xb, yb, xnb, ynb, norm=norm)
    want_c, want_n = [], []
    for b in range(2):
        p, q, pn, qn = (t[b].cpu().numpy() for t in (xb, yb, xnb, ynb))
        ipq = metrics.nearest_points(xb[b], yb[b], norm)[1].cpu().numpy()
        iqp = metrics.nearest_points(yb[b], xb[b], norm)[1].cpu().numpy()
        d_pq, o_pq, s_pq = CO.nearest(p, q, norm, device=DEV); d_qp, o_qp, s_qp = CO.nearest(q, p, norm, device=DEV)
        for got, o, d1, d2 in ((ipq, o_pq, d_pq, s_pq), (iqp, o_qp, d_qp, s_qp)):       # these indices are validated here
            clear = d2 > (1.0 + 1e-5) * d1
            assert np.array_equal(got[clear], o[clear]) and clear.mean() >= 0.999
        assert (CO.pair_distance(p, q[ipq], norm) - d_pq <= 16 * U * d_pq).all()
        assert (CO.pair_distance(q, p[iqp], norm) - d_qp <= 16 * U * d_qp).all()
        want_c.append(d_pq.mean() + d_qp.mean())
        want_n.append(CO.normal_term(pn, qn, ipq).mean() + CO.normal_term(qn, pn, iqp).mean())
    want_c, want_n = float(np.mean(want_c)), float(np.mean(want_n))
    print(f"norm {norm}, batch of 2: cham_dist rel {abs(float(cdb) - want_c) / want_c:.2e}, cham_normals abs {abs(float(ncb) - want_n):.2e}")
    assert abs(float(cdb) - want_c) <= 1e-6 * want_c and abs(float(ncb) - want_n) <= 2e-6
    cdb1, ncb1 = metrics.chamfer_distance(xb[:1], yb[:1], xnb[:1], ynb[:1], norm=norm)
    cdb0, ncb0 = metrics.chamfer_distance(xb[0], yb[0], xnb[0], ynb[0], norm=norm)
    assert float(cdb1) == float(cdb0) and float(ncb1) == float(ncb0)
    # a cloud against itself
    cds, ncs = metrics.chamfer_distance(xd, xd, xnd, xnd, norm=norm)
    assert float(cds) == 0.0 and -1e-12 <= float(ncs) <= 2e-6             # (a cosine of 1 rounds to either side of it)


def _golden_cap_mesh():
    """TriangleSoup of the trained 4 x 128 network of tests/golden/g14_pointcloud.npz, CAP-UDF at 64^3."""
    from diffudf_amd.model import SIREN
    from diffudf_amd.render_mc import TriangleSoup, extract_fields, extract_mesh_CAP
    G = np.load(os.path.join(HERE, "golden", "g14_pointcloud.npz"))
    m = SIREN(3, 1, [128] * 4, w0=30).cuda()
    with torch.no_grad():
        m.flat_parameters().copy_(_cuda(G["t_theta"]))
    df, vec = extract_fields(m, None, 64, "tanh", torch.device(DEV), float(G["alpha"]))
    mesh = extract_mesh_CAP(df, vec, 64)
    return TriangleSoup(np.asarray(mesh.vertices), np.asarray(mesh.faces))


def test_vertex_normals(beetle):
    from diffudf_amd import metrics
    from diffudf_amd.render_mc import TriangleSoup
    v, t = beetle
    soup = _golden_cap_mesh()
    assert len(soup.vertices) > 1000 and len(soup.faces) > 1000
    for name, vv, ff in (("beetle", v, t), ("cap", soup.vertices, soup.faces)):
        got = metrics.vertex_normals(_cuda(vv), _cuda(ff))
        assert got.dtype == torch.float32 and got.shape == (len(vv), 3) and got.is_cuda
        want = CO.vertex_normals(vv, ff)
        err = float(np.abs(got.cpu().numpy() - want).max())
        print(f"vertex normals, {name}: {len(vv)} vertices, {len(ff)} faces, max component error {err:.2e}")
        assert err <= 1e-6
    prop = soup.vertex_normals                                            # the added attribute of TriangleSoup
    assert prop.shape == soup.vertices.shape and np.abs(prop - CO.vertex_normals(soup.vertices, soup.faces)).max() <= 1e-6
    # an unreferenced vertex gives (0, 0, 1); a face with an index out of range is skipped
    v2 = np.concatenate([v[:100], [[9.0, 9.0, 9.0]]]); keep = t[(t < 100).all(1)]
    f2 = np.concatenate([keep, [[0, 1, 101], [-1, 2, 3], [5, 6, 1 << 40]]])
    got = metrics.vertex_normals(_cuda(v2), _cuda(f2)).cpu().numpy()
    assert got[100].tolist() == [0.0, 0.0, 1.0]
    assert np.abs(got - CO.vertex_normals(v2, keep)).max() <= 1e-6
    empty = TriangleSoup(v[:5], np.zeros((0, 3), np.int64)).vertex_normals
    assert empty.tolist() == [[0.0, 0.0, 1.0]] * 5


def test_cuantitative_end_to_end(tmp_path, beetle, capsys):
    import cuantitative
    from diffudf_amd import mesh
    v, t = beetle
    data = tmp_path / "data" / "beetle"; out = tmp_path / "results"
    os.makedirs(data)
    pos, nrm = mesh.sample_surface(v, t, 20000, seed=3)
    mesh.write_obj(str(data / "beetle_t.obj"), v, t)
    mesh.write_ply_points(str(data / "beetle_pc.ply"), pos, nrm)
    cfg = cuantitative.default_exp_config(str(out))
    cfg.update({"num_epochs": 120, "s1_epochs": 80, "warmup_epochs": 40, "batch_size": 6000, "resolution": 48,
                "network": {"hidden_layer_nodes": [64] * 4, "w0": 30, "pretrained_dict": "None"}})
    rows = cuantitative.run(str(tmp_path / "data"), str(out), 0, exp_config=cfg)
    lines = open(out / "results.csv").read().splitlines()
    assert lines[0] == "mesh,time,L1CD_CAP,L2CD_CAP,NC_CAP,L1CD_MU,L2CD_MU,NC_MU" and len(lines) == 2 and len(rows) == 1
    cells = lines[1].split(",")
    assert cells[0] == "beetle" and len(cells) == 8 and float(cells[1]) > 0
    cap = np.array([float(c) for c in cells[2:5]]); mu = np.array([float(c) for c in cells[5:8]])
    assert np.isfinite(cap).all() and (cap >= 0).all()
    mesh_mu, mesh_cap = rows[0][8]
    pc = cuantitative.PointCloudFile(str(data / "beetle_pc.ply"))
    ev = cuantitative.EvalMesh(mesh_cap, 0)
    l1, nc = cuantitative.metrics(ev, pc, 1, 0); l2, _ = cuantitative.metrics(ev, pc, 2, 0)
    assert isinstance(l1, np.ndarray) and l1.shape == () and l1.dtype == np.float32
    assert [float(l1), float(l2), float(nc)] == [float(c) for c in cells[2:5]]
    # a mesh without vertex normals of its own: computed from its faces, the same numbers
    class Bare:
        vertices, faces = ev.vertices, ev.faces
    assert float(cuantitative.metrics(Bare, pc, 1, 0)[1]) == float(cells[4])
    # against the oracle at the device's indices
    want_cd, _ = CO.chamfer(ev.vertices.astype(np.float32), pc.points, 2, device=DEV)
    assert abs(float(l2) - want_cd) <= 1e-6 * want_cd
    if mesh_mu is None:
        assert np.isnan(mu).all()
    else:
        assert np.isfinite(mu).all()
    # a second run skips the experiment whose folder exists: header only
    assert cuantitative.run(str(tmp_path / "data"), str(out), 0, exp_config=cfg) == []
    assert open(out / "results.csv").read().splitlines() == [lines[0]]


def _bench_tool():
    """tools/bench_chamfer.py as a module: the test and the tool time the same baseline with the same code."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_chamfer", os.path.join(os.path.dirname(HERE), "tools", "bench_chamfer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("norm", [1, 2])
def test_faster_than_chunked_torch(beetle, norm):
    """One direction at 100 000 x 100 000, warmed, median of 7, events on the stream; the baseline runs in the same process on the
    same GPU.  The kernel must be faster."""
    from diffudf_amd import mesh, metrics
    tool = _bench_tool()
    torch_nearest, _time_ms = tool.torch_nearest, lambda fn: tool.time_ms(fn, 7)[0]
    v, t = beetle
    x = _cuda(mesh.sample_surface(v, t, 100000, seed=1)[0]); y = _cuda(mesh.sample_surface(v, t, 100000, seed=2)[0])
    d, i = metrics.nearest_points(x, y, norm)
    db, ib = torch_nearest(x, y, norm)
    assert float((i == ib).float().mean()) >= 0.999                        # the two searches agree (near-ties aside)
    t_hip = _time_ms(lambda: metrics.nearest_points(x, y, norm))
    t_ref = _time_ms(lambda: torch_nearest(x, y, norm))
    # the same composition with 1 GiB handed to every cdist call (no cap on the pairs of a launch, see torch_nearest): whatever that
    # launch computes, the kernel is held against its time as well
    t_big = _time_ms(lambda: torch_nearest(x, y, norm, max_pairs=1 << 62))
    print(f"nearest 100000 x 100000 norm {norm}: HIP {t_hip:.3f} ms, chunked torch.cdist + min {t_ref:.3f} ms, ratio {t_ref / t_hip:.1f}; "
          f"with 1 GiB per cdist call {t_big:.3f} ms, ratio {t_big / t_hip:.1f}")
    assert t_ref / t_hip > 1.0 and t_big / t_hip > 1.0
