# coding: utf-8
"""GPU: the batch sampler through a BVH (csrc/dudf_sample_indexed.hip, csrc/dudf_groupwalk.h; `PointCloud(..., index="tree")`).

The pin is bit equality: from the same constructor arguments and step, `index="tree"` gives the triple (x, normals, sdf) of
`index="brute"` — `torch.equal` on all three, no tolerance.  Neither the minimum of exact fp64 values nor the one rounding of its
square root depends on how the search went."""
import ctypes
import os

import numpy as np
import pytest
import torch

import meshdist_oracle as MO
from diffudf_amd import _lib, hip_ops, mesh, synth
from oracle import sampler_oracle as SO

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BEETLE = os.path.join(HERE, "golden", "beetle")
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same(a, b):
    return all(torch.equal(u, v) for u, v in zip(a, b))


def pair(prefix=BEETLE, batch=3000, seed=7, **kw):
    """(brute, tree): two samplers from the same constructor arguments."""
    from diffudf_amd.dataset import PointCloud
    make = lambda index: PointCloud(prefix, batch, [0.333, 0.666], 1, device=DEV, seed=seed, index=index, **kw)  # noqa: E731
    return make("brute"), make("tree")


# ---- the beetle mesh: 2 053 triangles, 257 leaves, L = 512 with empty slots ---------------------------------------------------------
@pytest.fixture(scope="module")
def beetle():
    brute, tree = pair()
    assert brute.tri.shape == (2053, 9) and brute.index == "brute" and tree.index == "tree"
    assert brute._mesh_index is None and tree._mesh_index is not None and tree._cloud_index is None
    assert tree._mesh_index.numel() == _lib.load().dudf_mesh_index_bytes(2053)
    return brute, tree


@pytest.mark.parametrize("step", [0, 5, 6])
def test_beetle_tree_equals_brute(beetle, step):
    brute, tree = beetle
    b, t = brute.sample(step), tree.sample(step)
    assert t[0].shape == (2997, 3) and same(b, t)
    assert (t[2][:999] == 0).all() and (t[2][999:] > 0).all()


def test_beetle_shards_and_oracle(beetle):
    """rank 1 of 3 gives its slices of the global batch — the brute sampler's, the oracle's — and the union over world = 2 is the
    batch."""
    brute, tree = beetle
    b3, t3 = pair(rank=1, world=3)
    xs, ns, ss = t3.sample(5)
    assert same(b3.sample(5), (xs, ns, ss))
    full = tree.sample(5)
    for m in range(3):                                           # its [333, 666) of every stratum of 999
        assert same([v[999 * m + 333:999 * m + 666] for v in full], [v[333 * m:333 * (m + 1)] for v in (xs, ns, ss)])
    tri, pos, pn = t3.tri.cpu().numpy(), t3.pc_pos.cpu().numpy(), t3.pc_nrm.cpu().numpy()
    xo, no, so = SO.sample_batch(tri, pos, pn, 999, 999, 999, seed=7, step=5, rank=1, world=3)
    print("oracle: max |x - xo|", np.abs(xs.cpu().numpy() - xo).max(), "max |sdf - so|", np.abs(ss.cpu().numpy() - so[:, 0]).max())
    assert np.abs(xs.cpu().numpy() - xo).max() < 1e-6 and np.array_equal(ns.cpu().numpy(), no)
    assert np.abs(ss.cpu().numpy() - so[:, 0]).max() < 2e-6
    parts = [pair(rank=r, world=2)[1].sample(5) for r in range(2)]
    for k in range(3):
        got = torch.cat([torch.cat([parts[0][k][:499], parts[1][k][:500]]),
                         torch.cat([parts[0][k][499:998], parts[1][k][500:1000]]),
                         torch.cat([parts[0][k][998:], parts[1][k][1000:]])])
        assert torch.equal(got, full[k])


# ---- the beetle as a cloud ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("points", [5000, 100000])               # 100 000: the scan's second and later tiles
def test_beetle_cloud_tree_equals_brute(points):
    brute, tree = pair(seed=11, onlyPCloud=True, surfacePoints=points)
    assert tree.tri is None and tree._mesh_index is None and tree._cloud_index.numel() == _lib.load().dudf_cloud_index_bytes(points)
    stats = torch.zeros(1, dtype=torch.int64, device=DEV)
    b, t = brute.sample(2), tree.sample(2, stats=stats)
    assert same(b, t)
    assert (t[2][999:] > 0).all()
    assert 999 <= int(stats.item()) < 0.25 * 999 * points         # only the far stratum walks; near sdf = |offset|
    assert same(brute.sample(3), tree.sample(3))


def test_auto_picks_by_the_measured_thresholds(monkeypatch):
    from diffudf_amd import dataset
    make = lambda **kw: dataset.PointCloud(BEETLE, 3000, [0.333, 0.666], 1, device=DEV, seed=11, surfacePoints=5000, index="auto", **kw)  # noqa: E731
    assert make().index == "brute" and make(onlyPCloud=True).index == "brute"        # 2 053 triangles, 5 000 points: the scan
    monkeypatch.setattr(dataset, "AUTO_TREE_MIN_POINTS", 5000)
    monkeypatch.setattr(dataset, "AUTO_TREE_MIN_TRIANGLES", 2054)
    ds = make(onlyPCloud=True)
    assert ds.index == "tree" and ds._cloud_index is not None and make().index == "brute"
    monkeypatch.setattr(dataset, "AUTO_TREE_MIN_TRIANGLES", 2053)
    assert make().index == "tree"


# ---- tree-shape edges through the C ABI -------------------------------------------------------------------------------------------------
SIZES = [1, 7, 8, 9, 64, 65]
# (n_on, n_far, n_near): a partial last workgroup (75 samples x 8 lanes = 2 workgroups and 88 threads), no far stratum, no near
# stratum with on-surface samples, and more than one workgroup of queries
BATCHES = [(5, 40, 30), (7, 0, 20), (9, 33, 0), (0, 70, 0), (40, 100, 101)]


def unit(n, seed):
    v = np.stack([synth.uniform01(seed, 730 + k, 0, n) * 2.0 - 1.0 for k in range(3)], axis=1) + 1e-3
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def planted_soup(T, seed):
    """T small random triangles; from 2 on the last repeats the first, from 3 on the second is a needle (its corners collinear up
    to rounding), from 4 on the third has collapsed to a point (zero area exactly)."""
    c = np.stack([synth.uniform01(seed, 710 + k, 0, T) * 2.0 - 1.0 for k in range(3)], axis=1)
    e = np.stack([synth.uniform01(seed, 720 + k, 0, T * 3) for k in range(3)], axis=1).reshape(T, 3, 3) * 0.3 - 0.15
    tri = (c[:, None, :] + e).astype(np.float32)
    if T >= 3:
        tri[1, 2] = tri[1, 0] + np.float32(0.5) * (tri[1, 1] - tri[1, 0])
        tri[1, 1] = tri[1, 0] + np.float32(2.0) * (tri[1, 2] - tri[1, 0])
    if T >= 4:
        tri[2, 1] = tri[2, 0]; tri[2, 2] = tri[2, 0]
    if T >= 2:
        tri[T - 1] = tri[0]
    return tri.reshape(T, 9)


def planted_cloud(n, seed, coincident):
    """n random points with exact duplicates (every third point repeats point 0 or 1), or n copies of one point."""
    p = np.stack([synth.uniform01(seed, 740 + k, 0, n) * 1.8 - 0.9 for k in range(3)], axis=1).astype(np.float32)
    if coincident:
        p[:] = p[0]
    else:
        p[2::3] = p[(np.arange(2, n, 3) // 3) % 2]
    return p


def both_calls(tri, pos, nrm, batch, seed=19, step=4, rank=0, world=1, at=False):
    """((x, normals, sdf) of dudf_sample_batch, of dudf_sample_batch_indexed, exact evaluations) on the same arguments."""
    lib = _lib.load()
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    n_tri = 0 if tri is None else tri.shape[0]
    mesh_index = hip_ops.mesh_index_build(tri) if n_tri else None
    cloud_index = None if n_tri else hip_ops.cloud_index_build(pos)
    sl = lambda m: m * (rank + 1) // world - m * rank // world  # noqa: E731
    n = sum(sl(m) for m in batch)
    out = [[torch.full((n, 3), 7.0, device=DEV), torch.full((n, 3), 7.0, device=DEV), torch.full((n,), 7.0, device=DEV)] for _ in range(2)]
    stats = torch.zeros(1, dtype=torch.int64, device=DEV)
    step_dev = torch.full((1,), step, dtype=torch.int64, device=DEV)
    head = (P(tri), n_tri, P(pos), P(nrm), pos.shape[0], *batch, seed, P(step_dev) if at else step, rank, world)
    B = lambda t: (P(t), t.numel()) if t is not None else (None, 0)  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = (lib.dudf_sample_batch_at if at else lib.dudf_sample_batch)(*head, *[P(t) for t in out[0]], st)
    assert rc == 0, rc
    rc = (lib.dudf_sample_batch_indexed_at if at else lib.dudf_sample_batch_indexed)(*head, *B(mesh_index), *B(cloud_index),
                                                                                    *[P(t) for t in out[1]], P(stats), st)
    assert rc == 0, rc
    return out[0], out[1], int(stats.item())


@pytest.mark.parametrize("T", SIZES)
def test_planted_soups(T):
    tri = dev(planted_soup(T, 100 + T))
    pos = dev(planted_cloud(50, 3, False)); nrm = dev(unit(50, 4))
    for k, batch in enumerate(BATCHES):
        b, t, evals = both_calls(tri, pos, nrm, batch, step=k, at=(k == 1))
        assert same(b, t), (T, batch)
        queries = batch[1] + batch[2]
        assert queries * min(T, 1) <= evals <= queries * T, (T, batch, evals)     # every query meets a leaf; nothing is met twice
        assert (t[2][:batch[0]] == 0).all() and (t[2][batch[0]:] > 0).all()
    b, t, _ = both_calls(tri, pos, nrm, BATCHES[4], rank=1, world=3)
    assert same(b, t)


@pytest.mark.parametrize("coincident", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_planted_clouds(n, coincident):
    pos = dev(planted_cloud(n, 200 + n, coincident)); nrm = dev(unit(n, 5))
    for k, batch in enumerate(BATCHES):
        b, t, evals = both_calls(None, pos, nrm, batch, step=k, at=(k == 2))
        assert same(b, t), (n, batch)
        assert batch[1] <= evals <= batch[1] * n, (n, batch, evals)                # the far stratum alone walks
    b, t, _ = both_calls(None, pos, nrm, BATCHES[4], rank=2, world=3)
    assert same(b, t)


def test_two_cloud_builds_are_byte_identical():
    pos = dev(planted_cloud(1000, 9, False))
    a, b = hip_ops.cloud_index_build(pos), hip_ops.cloud_index_build(pos)
    assert torch.equal(a, b)
    rows = a[256:256 + 16 * 1000].view(torch.float32).reshape(1000, 4)            # the sorted copy: a permutation of the points
    assert torch.equal(rows[:, 3], torch.zeros(1000, device=DEV))
    key = lambda p: p[:, :3].contiguous().cpu().numpy().view([("", np.float32)] * 3).ravel()  # noqa: E731
    assert np.array_equal(np.sort(key(rows)), np.sort(key(pos)))


# ---- a generated icosphere, level 5: 20 480 triangles -----------------------------------------------------------------------------------
def test_icosphere_tree_equals_brute_and_prunes(tmp_path):
    v, f = MO.bench_meshdist.icosphere(5)
    v = v / 1.1
    prefix = str(tmp_path / "sphere")
    mesh.write_obj(prefix + "_t.obj", v, f, fmt="%.17g")
    brute, tree = pair(prefix, surfacePoints=20000)
    assert tree.tri.shape == (20480, 9)
    stats = torch.zeros(1, dtype=torch.int64, device=DEV)
    b, t = brute.sample(1), tree.sample(1, stats=stats)
    assert same(b, t)
    queries = 2997 - 999
    frac = int(stats.item()) / (queries * 20480)
    print(f"icosphere: {int(stats.item()) / queries:.1f} evaluations per query, {100 * frac:.2f} % of the scan")
    assert 0 < frac < 0.25


# ---- graph replay ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("only_cloud", [False, True])
def test_tree_sampler_replays_in_a_graph(only_cloud):
    a, b = pair(batch=6000, seed=123, onlyPCloud=only_cloud, surfacePoints=20000)      # a: brute, eager; b: tree, replayed
    for _ in range(3):
        next(iter(a)); next(iter(b))
    b.use_device_step()                                          # picks up at step 3
    xa, na, sa = next(iter(a)); xb, nb, sb = next(iter(b))
    assert torch.equal(xa, xb) and torch.equal(na, nb) and torch.equal(sa, sb)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                    # raises if the call synchronised or allocated through the runtime
        xg, ng, sg = next(iter(b))
    for _ in range(3):
        g.replay()
        xa, na, sa = next(iter(a))
        assert torch.equal(xa, xg) and torch.equal(na, ng) and torch.equal(sa, sg)
    assert a._step == 7 and int(b._step_dev.item()) == 7


# ---- the flag ---------------------------------------------------------------------------------------------------------------------------
def test_a_nan_vertex_is_refused_at_construction(tmp_path):
    from diffudf_amd.dataset import PointCloud
    v, f = MO.bench_meshdist.icosphere(1)
    v = v / 1.1
    pos, nrm = mesh.sample_surface(v, f, 500, 3)
    prefix = str(tmp_path / "bad")
    mesh.write_ply_points(prefix + "_pc.ply", pos, nrm)
    v[17, 1] = np.nan
    mesh.write_obj(prefix + "_t.obj", v, f)
    args = (prefix, 3000, [0.333, 0.666], 1)
    PointCloud(*args, device=DEV)                                # the scan does not look
    with pytest.raises(ValueError, match="NaN"):
        PointCloud(*args, device=DEV, index="tree")
    pos[3, 0] = np.inf
    mesh.write_ply_points(prefix + "_pc.ply", pos, nrm)
    with pytest.raises(ValueError, match="NaN"):
        PointCloud(*args, device=DEV, onlyPCloud=True, index="tree")
