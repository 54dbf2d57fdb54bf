# coding: utf-8
"""CPU: the refusals of the indexed batch sampler and of the cloud index (include/dudf_hip.h), and train.py's `sampler_index` key.

Every call here returns before its first HIP call, as in tests/test_cabi_errors.py: the "device" pointers are a host address that is
never dereferenced, the index a 256-byte-aligned host buffer."""
import ctypes

import pytest

from diffudf_amd import _lib

OK, E_CFG, E_WS, E_MODE, E_UNSUP = 0, -1, -2, -3, -4
T, NPC = 65, 100                                        # triangles / cloud points of every call

_arena = ctypes.create_string_buffer(1 << 20)
BASE = (ctypes.addressof(_arena) + 255) // 256 * 256
P = ctypes.c_void_p(BASE)                               # stands in for any device pointer (never read)


def sizes():
    lib = _lib.load()
    return int(lib.dudf_mesh_index_bytes(T)), int(lib.dudf_cloud_index_bytes(NPC))


def call(at=False, tri=P, n_tri=T, pos=P, nrm=P, n_pc=NPC, n_on=10, n_far=10, n_near=10, step=3, rank=0, world=1, mesh=None,
         cloud=None):
    """dudf_sample_batch_indexed(_at) with the given (pointer, bytes) pairs; step=None: a null step pointer for the _at form."""
    lib = _lib.load()
    mesh = mesh if mesh is not None else (None, 0)
    cloud = cloud if cloud is not None else (None, 0)
    fn = lib.dudf_sample_batch_indexed_at if at else lib.dudf_sample_batch_indexed
    step_arg = (P if step is not None else None) if at else step
    return fn(tri, n_tri, pos, nrm, n_pc, n_on, n_far, n_near, 7, step_arg, rank, world, mesh[0], mesh[1], cloud[0], cloud[1],
              P, P, P, None, None)


def test_cloud_index_bytes_is_zero_out_of_range():
    lib = _lib.load()
    assert lib.dudf_cloud_index_bytes(0) == 0
    assert lib.dudf_cloud_index_bytes(-5) == 0
    assert lib.dudf_cloud_index_bytes(1 << 31) == 0
    # header, the 16-byte rows, the boxes of 2 L - 1 nodes (L = 16 leaf slots for 13 leaves), each on a 256-byte granule
    assert lib.dudf_cloud_index_bytes(NPC) == 256 + (NPC * 16 + 255) // 256 * 256 + (31 * 32 + 255) // 256 * 256
    assert lib.dudf_cloud_index_bytes(1) == 256 + 256 + 256
    assert lib.dudf_cloud_index_bytes((1 << 31) - 1) > 0


@pytest.mark.parametrize("name", ["dudf_cloud_morton_codes", "dudf_cloud_index_build"])
def test_cloud_index_refusals_follow_the_mesh_index(name):
    lib = _lib.load()
    nb = sizes()[1]
    if name == "dudf_cloud_morton_codes":
        f = lambda pos=P, n=NPC, ws=P, nbytes=nb, out=P: lib.dudf_cloud_morton_codes(pos, n, ws, nbytes, out, None)  # noqa: E731
    else:
        f = lambda pos=P, n=NPC, ws=P, nbytes=nb, out=P: lib.dudf_cloud_index_build(pos, n, out, ws, nbytes, None)  # noqa: E731
    assert f(n=0) == E_CFG and f(n=-1) == E_CFG
    assert f(pos=None) == E_CFG
    assert f(out=None) == E_CFG                           # the codes / the order
    assert f(n=1 << 31, ws=None, nbytes=0) == E_UNSUP
    assert f(ws=None) == E_WS
    assert f(ws=ctypes.c_void_p(BASE + 8)) == E_WS
    assert f(nbytes=nb - 1) == E_WS
    assert f(pos=None, ws=None) == E_CFG                  # the arguments before the buffer


@pytest.mark.parametrize("at", [False, True])
def test_the_refusals_of_sample_batch_come_first(at):
    mb, cb = sizes()
    good = dict(at=at, mesh=(P, mb))
    assert call(**good, n_tri=-1) == E_CFG
    assert call(**good, tri=None) == E_CFG
    assert call(**good, n_pc=0) == E_CFG
    assert call(**good, world=0) == E_CFG
    assert call(**good, rank=-1) == E_CFG
    assert call(**good, rank=2, world=2) == E_CFG
    assert call(**good, n_on=-1) == E_CFG
    assert call(**good, n_far=-1) == E_CFG
    assert call(**good, n_near=-1) == E_CFG
    assert call(**good, n_on=0, n_near=4) == E_CFG
    assert call(at=at, n_pc=0, mesh=(None, 0)) == E_CFG   # ... also ahead of the index
    assert call(at=at, n_pc=0, mesh=(P, mb - 1)) == E_CFG
    if at:
        assert call(**good, step=None) == E_CFG


@pytest.mark.parametrize("at", [False, True])
def test_index_refusals(at):
    mb, cb = sizes()
    # mesh input needs the mesh index, cloud input (n_tri == 0) the cloud index; the other pair is not looked at
    assert call(at=at) == E_CFG                                             # a mesh and no index at all
    assert call(at=at, cloud=(P, cb)) == E_CFG                              # ... and the wrong one does not help
    assert call(at=at, n_tri=0, tri=None) == E_CFG
    assert call(at=at, n_tri=0, tri=None, mesh=(P, mb)) == E_CFG
    for kw, nb in ((dict(), mb), (dict(n_tri=0, tri=None), cb)):
        pair = "cloud" if kw else "mesh"
        assert call(at=at, **kw, **{pair: (None, nb)}) == E_WS              # missing
        assert call(at=at, **kw, **{pair: (ctypes.c_void_p(BASE + 16), nb)}) == E_WS
        assert call(at=at, **kw, **{pair: (ctypes.c_void_p(BASE + 128), nb)}) == E_WS
        assert call(at=at, **kw, **{pair: (P, nb - 1)}) == E_WS             # the wrong size, either way
        assert call(at=at, **kw, **{pair: (P, nb + 256)}) == E_WS
        assert call(at=at, **kw, **{pair: (P, 0)}) == E_WS
    assert call(at=at, mesh=(P, cb)) == E_WS                                # the cloud's size for the mesh's index
    assert call(at=at, n_tri=1 << 31, mesh=(P, mb)) == E_UNSUP
    assert call(at=at, n_tri=0, tri=None, n_pc=1 << 31, cloud=(P, cb)) == E_UNSUP


@pytest.mark.parametrize("at", [False, True])
def test_an_empty_slice_is_accepted_before_any_device_call(at):
    """rank 0 of 4 of a batch of (1, 1, 1) owns nothing: every check passes and nothing is launched."""
    mb, cb = sizes()
    assert call(at=at, n_on=1, n_far=1, n_near=1, rank=0, world=4, mesh=(P, mb)) == OK
    assert call(at=at, n_tri=0, tri=None, n_on=0, n_far=0, n_near=0, cloud=(P, cb)) == OK


def test_train_rejects_an_unknown_sampler_index_by_name():
    import train
    assert train.sampler_index_of({}) == "brute"
    for mode in ("brute", "tree", "auto"):
        assert train.sampler_index_of({"sampler_index": mode}) == mode
    with pytest.raises(ValueError, match="sampler_index"):
        train.sampler_index_of({"sampler_index": "kdtree"})
    with pytest.raises(ValueError, match="sampler_index"):            # before anything else of the run is set up
        train.setup_train({"sampler_index": True}, 0)


def test_pointcloud_rejects_an_unknown_index_before_it_loads_anything():
    from diffudf_amd.dataset import PointCloud
    with pytest.raises(ValueError, match="index"):
        PointCloud("/nonexistent/prefix", 3000, [0.333, 0.666], 1, device="cuda:0", index="bvh")
