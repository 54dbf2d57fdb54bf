# coding: utf-8
"""GPU: the bytes of the two Morton-tree indexes (`dudf_mesh_index_build`, `dudf_cloud_index_build`) and their Morton codes against a
numpy statement of the published layout — include/dudf_hip.h and the head of csrc/dudf_bvh.h; nothing here calls the library to
say what the bytes should be.

The layout, every section on a 256-byte granule, zero where nothing is written:
  header   uint32[64]: words 0..2 / 3..5 = min / max of all coordinates as order-preserving codes, word 6 (byte 24) = flags;
  mesh     ids int32[n] (order), the sorted triangles float32[n][9], nodes float32[2L - 1][8];
  cloud    the sorted points float32[n][4] = (x, y, z, 0), nodes float32[2L - 1][8];
  nodes    heap order over L = the leaf count (8 primitives a leaf) rounded up to a power of two, a node = (lo.xyz hi.x | hi.yz 0 0),
           an empty leaf slot = (lo +inf, hi -inf), a parent = min / max of its two children.
Codes: per axis q = (key - lo) / ext * 2^21 in fp64 (0 for a zero extent), clamped to [0, 2^21 - 1], truncated; bit i of the x, y,
z cell at bit 3 i + 2, 3 i + 1, 3 i.  key = the point's coordinate, or the fp64 centroid ((a + b) + c) * (1 / 3) of a triangle,
whose product the device fuses with the subtraction of lo (one rounding; stated here with exact rationals).
Sizes 1 (the root is the leaf), 7 / 8 / 9 (the leaf edge), 64 / 65 (L 8 -> 16: seven empty slots)."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from diffudf_amd import _lib, hip_ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [1, 7, 8, 9, 64, 65]
KINDS = ["mesh", "cloud"]


def planted(kind, n, case="random"):
    """(n, 9) triangles or (n, 3) points, float32."""
    w = 9 if kind == "mesh" else 3
    rng = np.random.default_rng(1000 * n + w)
    a = rng.uniform(-1.0, 1.0, (n, w)).astype(np.float32)
    if case == "plane":                                   # z = 0.25 everywhere: a zero extent
        a[:, 2::3] = np.float32(0.25)
    elif case == "duplicates":                            # three distinct primitives, each three times: equal codes
        a = a[np.arange(n) % 3]
    elif case == "nan":
        a[n // 2, 1] = np.nan
    return np.ascontiguousarray(a)


def float_code(f):
    b = np.asarray(f, np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def oracle_codes(kind, a):
    xyz = a.reshape(-1, 3)
    lo = xyz.min(0).astype(np.float64)
    ext = xyz.max(0).astype(np.float64) - lo
    d = a.astype(np.float64)
    if kind == "mesh":                                    # the device fuses centroid and offset: sum * (1 / 3) - lo, rounded once
        third, s = Fraction(1.0 / 3.0), (d[:, 0:3] + d[:, 3:6]) + d[:, 6:9]
        off = np.array([[float(Fraction(v) * third - Fraction(l)) for v, l in zip(row, lo)] for row in s]).reshape(-1, 3)
    else:
        off = d - lo
    code = np.zeros(len(a), np.uint64)
    for ax in range(3):
        q = off[:, ax] / ext[ax] * 2097152.0 if ext[ax] > 0.0 else np.zeros(len(a))
        q = np.minimum(np.maximum(q, 0.0), 2097151.0).astype(np.uint64)
        for i in range(21):
            code |= ((q >> np.uint64(i)) & np.uint64(1)) << np.uint64(3 * i + 2 - ax)
    return code.astype(np.int64)


def granule(x):
    b = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
    return np.concatenate([b, np.zeros(-len(b) % 256, np.uint8)])


def oracle_index(kind, a, order):
    n = len(a)
    xyz = a.reshape(-1, 3)
    hdr = np.zeros(64, np.uint32)
    hdr[0:3], hdr[3:6] = float_code(xyz.min(0)), float_code(xyz.max(0))
    L = 1
    while L * 8 < n:
        L *= 2
    s = a[order]
    nodes = np.zeros((2 * L - 1, 8), np.float32)
    nodes[:, 0:3], nodes[:, 3:6] = np.inf, -np.inf
    for j in range((n + 7) // 8):
        v = s[8 * j:8 * j + 8].reshape(-1, 3)
        nodes[L - 1 + j, 0:3], nodes[L - 1 + j, 3:6] = v.min(0), v.max(0)
    for i in range(L - 2, -1, -1):
        nodes[i, 0:3] = np.minimum(nodes[2 * i + 1, 0:3], nodes[2 * i + 2, 0:3])
        nodes[i, 3:6] = np.maximum(nodes[2 * i + 1, 3:6], nodes[2 * i + 2, 3:6])
    if kind == "mesh":
        prims = [granule(order.astype(np.int32)), granule(s)]
    else:
        prims = [granule(np.concatenate([s, np.zeros((n, 1), np.float32)], 1))]
    return np.concatenate([granule(hdr)] + prims + [granule(nodes)])


def device_codes(kind, a):
    """(codes, index): the Morton codes of the library and the buffer whose head it used as scratch."""
    t = torch.from_numpy(a).to(DEV)
    n = len(a)
    nbytes = int(getattr(_lib.load(), f"dudf_{kind}_index_bytes")(n))
    index = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    codes = torch.empty(n, dtype=torch.int64, device=DEV)
    hip_ops._call(f"dudf_{kind}_morton_codes", hip_ops._ptr(t), n, hip_ops._ptr(index), nbytes, hip_ops._ptr(codes))
    return codes.cpu().numpy(), index, t


def build(kind, a, order=None):
    f = hip_ops.mesh_index_build if kind == "mesh" else hip_ops.cloud_index_build
    o = None if order is None else torch.from_numpy(np.ascontiguousarray(order)).to(DEV)
    return f(torch.from_numpy(a).to(DEV), o).cpu().numpy()


def check(kind, a):
    codes = oracle_codes(kind, a)
    got = device_codes(kind, a)[0]
    assert np.array_equal(got, codes), (got, codes)
    for order, given in ((np.argsort(codes, kind="stable"), None), (np.arange(len(a))[::-1].copy(), True)):
        want = oracle_index(kind, a, order)
        index = build(kind, a, order if given else None)
        assert index.shape == want.shape, (index.shape, want.shape)
        bad = np.flatnonzero(index != want)
        assert bad.size == 0, f"first differing byte {bad[0]} of {len(want)}"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_codes_and_index_bytes(kind, n):
    check(kind, planted(kind, n))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", ["plane", "duplicates"])
def test_planted_codes_and_index_bytes(kind, case):
    a = planted(kind, 9, case)
    codes = oracle_codes(kind, a)
    if case == "plane":
        assert not (codes & 0x1249249249249249).any()                 # the z bits
    else:
        assert len(np.unique(codes)) == 3                             # the stable sort decides among equals
    check(kind, a)


@pytest.mark.parametrize("kind", KINDS)
def test_nan_coordinate_sets_the_flag(kind):
    a = planted(kind, 9, "nan")
    _, index, t = device_codes(kind, a)
    order = torch.arange(9, dtype=torch.int64, device=DEV)
    hip_ops._call(f"dudf_{kind}_index_build", hip_ops._ptr(t), 9, hip_ops._ptr(order), hip_ops._ptr(index), index.numel())
    flags = int(index[hip_ops.MESH_INDEX_FLAGS_OFFSET:hip_ops.MESH_INDEX_FLAGS_OFFSET + 4].view(torch.int32).item())
    assert flags == hip_ops.MESH_FLAG_NONFINITE
    with pytest.raises(ValueError):
        build(kind, a)
