# coding: utf-8
"""One-off (round 5): the sampler's fp32-screened scan against the previous build's scan (dbg/r04: fp64 sphere test, same exact
arithmetic) — bit identity of every output at the reference's batch size, mesh and cloud-only — and the time of both.
The previous build is a worktree of the round-4 commit with its library built in place:
    git worktree add dbg/r04 9a5f2a9 && make -C dbg/r04/diffudf_amd/csrc
Record: profiles/r05_s_sampler_variants.txt."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                   # noqa: E402
from diffudf_amd.dataset import PointCloud     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
old = ctypes.CDLL(os.path.join(ROOT, "dbg", "r04", "diffudf_amd", "libdudf_hip.so"))
old.dudf_sample_batch.restype = ctypes.c_int
old.dudf_sample_batch.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                  ctypes.c_int64, ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
                                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]


def old_sample(ds, step):
    n = sum(ds.n_local())
    x = torch.empty(n, 3, device=ds.device); nr = torch.empty(n, 3, device=ds.device); sd = torch.empty(n, device=ds.device)
    rc = old.dudf_sample_batch(ds.tri.data_ptr() if ds.tri is not None else None, ds.tri.shape[0] if ds.tri is not None else 0,
                               ds.pc_pos.data_ptr(), ds.pc_nrm.data_ptr(), ds.pc_pos.shape[0], ds.samplesOnSurface, ds.n_far, ds.n_near,
                               ds.seed, step, ds.rank, ds.world, x.data_ptr(), nr.data_ptr(), sd.data_ptr(),
                               torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    return x, nr, sd


def timed(f, reps=30):
    for _ in range(3):
        f()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        f()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


for only in (False, True):
    for kw in ({}, {"rank": 1, "world": 3}):
        ds = PointCloud(os.path.join(ROOT, "tests", "golden", "beetle"), 30000, [0.333, 0.666], 1, device="cuda:0", onlyPCloud=only, **kw)
        same = True
        for step in (0, 1, 7, 123, 2999):
            a = ds.sample(step); b = old_sample(ds, step)
            same &= all(torch.equal(u, v) for u, v in zip(a, b))
        t_new = timed(lambda: ds.sample(3)); t_old = timed(lambda: old_sample(ds, 3))
        print(f"onlyPCloud={only} {kw or ''} triangles {0 if ds.tri is None else ds.tri.shape[0]} cloud {ds.pc_pos.shape[0]} points {sum(ds.n_local())}: "
              f"bit-identical {same}; new {t_new * 1e3:.1f} us, previous {t_old * 1e3:.1f} us", flush=True)
        assert same
