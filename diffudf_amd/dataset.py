# coding: utf-8
"""Batch source for the training loop, with the reference's yield contract (reference
src/dataset.py:134-185): an iterable whose `__iter__` yields `batchesPerEpoch` tuples

    coords (1,N,3), normals (1,N,3) [zeros off-surface], sdf (1,N,1) [zeros on-surface]     fp32, CPU

with N = int(B*p0) + 2*(int(B*p1)//2) points ordered [on-surface | far | near] (reference :162-163, :27-28).

This is also the SHARDING SEAM of the multi-GPU path: `rank`/`world` select this rank's equal slice of each
of the three strata, so every rank keeps the on/far/near mix and the union over ranks is the global batch.

`SyntheticPointCloud` draws the batch from `diffudf_amd.synth` (uniform coordinates, the same three strata);
`PointCloud` is the mesh-backed sampler: host-side OBJ/PLY preparation in
`diffudf_amd/mesh.py`, per-step sampling + exact point-to-triangle distance on the GPU (`csrc/dudf_sample.hip`: a scan of the
whole shape, the default path; `csrc/dudf_sample_indexed.hip`: through a BVH, for large meshes and clouds — `index="tree"`).
The reference's own one needs open3d, which this image does not have.
"""
import numpy as np
import torch

from . import synth


SAMPLER_INDEX_MODES = ("brute", "tree", "auto")
# `index="auto"`: the smallest measured sizes from which the tree's [min, max] time per batch lies wholly below the scan's
# (tools/bench_sampler_index.py on one MI355X, batch 30 000; the run is in profiles/HISTORY.md, "Sampler through a BVH").  Below
# them the scan stays.  None: no measured size qualified — up to 1 310 720 triangles (an icosphere) the tree's slowest batch was
# never below the scan's fastest, so "auto" keeps every mesh on the scan; clouds qualified at the 10^6 points measured (the
# next smaller size measured, 10^5, did not).
AUTO_TREE_MIN_TRIANGLES = None
AUTO_TREE_MIN_POINTS = 1000000


def check_sampler_index(index, key="index"):
    """`index` if it names a sampler mode, else ValueError naming `key` (the keyword, or the config key it came from)."""
    if index not in SAMPLER_INDEX_MODES:
        raise ValueError(f"{key}: {index!r} is not one of {', '.join(repr(m) for m in SAMPLER_INDEX_MODES)}")
    return index


def batch_size_of(batchSize, samplingPercentiles):
    n_on = int(batchSize * samplingPercentiles[0])
    n_off = int(batchSize * samplingPercentiles[1])
    return n_on + 2 * (n_off // 2)


class SyntheticPointCloud:
    def __init__(self, batchSize=30000, samplingPercentiles=(0.333, 0.666), batchesPerEpoch=1, seed=123,
                 rank=0, world=1):
        self.batchSize = batchSize
        self.samplingPercentiles = list(samplingPercentiles)
        self.batchesPerEpoch = batchesPerEpoch
        self.seed, self.rank, self.world = seed, rank, world
        self.n_global = batch_size_of(batchSize, samplingPercentiles)
        self._step = 0

    def local_indices(self):
        return synth.stratified_shard(self.n_global, self.rank, self.world)

    @property
    def n_on_surface(self):
        """Leading on-surface points of THIS rank's batch ([on | far | near]; train.py passes it to loss_s1 as a hint)."""
        return int((self.local_indices() < self.n_global // 3).sum())

    def __iter__(self):
        for _ in range(self.batchesPerEpoch):
            idx = self.local_indices()
            cuts = np.flatnonzero(np.diff(idx) != 1) + 1
            xs, ns, ss = [], [], []
            for part in np.split(idx, cuts):
                x, n, s = synth.training_batch(self.n_global, seed=self.seed, step=self._step, lo=int(part[0]),
                                               hi=int(part[-1]) + 1)
                xs.append(x); ns.append(n); ss.append(s)
            self._step += 1
            yield (torch.from_numpy(np.concatenate(xs))[None], torch.from_numpy(np.concatenate(ns))[None],
                   torch.from_numpy(np.concatenate(ss))[None])


class PointCloud:
    """Mesh-backed batch source with the reference constructor (reference src/dataset.py:135-155):
    `PointCloud(meshPath, batchSize, samplingPercentiles, batchesPerEpoch, device, onlyPCloud)`.

    `meshPath` is the reference's path prefix (`<prefix>_t.obj` + `<prefix>_pc.ply` as written by its preprocess.py);
    when those do not exist `<prefix>.obj` is normalised and sampled in memory (diffudf_amd/mesh.py).  Every batch is
    produced on the GPU by `dudf_sample_batch` and yielded as DEVICE tensors (the loop's `.to(device)` is then a
    no-op), ordered [on | far | near] exactly like the reference.  `rank`/`world` shard each stratum.
    `onlyPCloud=True` (point-cloud input, reference :80-131): only `<prefix>_pc.ply` (or the in-memory cloud) is used;
    far distances go to the nearest cloud point and near distances are |offset|.  A `_pc.ply` without normals (a raw scan) gets
    them estimated and oriented once at load (`metrics.estimate_normals`).
    `index`: how the off-surface distances are found — "brute" (default) scans the whole shape per batch (`dudf_sample_batch`);
    "tree" builds a BVH over the triangles (or, with onlyPCloud, over the cloud) once, here, and walks it
    (`dudf_sample_batch_indexed`; ValueError for a NaN or infinite coordinate); "auto" takes the tree from
    AUTO_TREE_MIN_TRIANGLES / AUTO_TREE_MIN_POINTS on.  The batches are bit-identical in every mode."""

    def __init__(self, meshPath, batchSize, samplingPercentiles, batchesPerEpoch, device=None, onlyPCloud=False,
                 seed=123, rank=0, world=1, surfacePoints=100000, index="brute"):
        import ctypes
        from . import _lib, mesh
        check_sampler_index(index)
        self.onlyPCloud = bool(onlyPCloud)
        self.device = torch.device("cuda", 0) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise _lib.DudfError("PointCloud: the sampler runs on the GPU; there is no CPU fallback path")
        tri, pos, nrm = mesh.prepare(meshPath, surfacePoints, seed, cloud_only=self.onlyPCloud, device=self.device)
        self.tri = None if self.onlyPCloud else torch.from_numpy(tri).to(self.device)
        self.pc_pos = torch.from_numpy(pos).to(self.device)
        self.pc_nrm = torch.from_numpy(nrm).to(self.device)
        self.batchSize, self.batchesPerEpoch = batchSize, batchesPerEpoch
        self.samplesOnSurface = int(batchSize * samplingPercentiles[0])
        self.samplesOffSurface = int(batchSize * samplingPercentiles[1])
        self.n_far = self.samplesOffSurface // 2
        self.n_near = self.samplesOffSurface - self.n_far
        self.n_global = self.samplesOnSurface + self.samplesOffSurface
        self.seed, self.rank, self.world = seed, rank, world
        self._step = 0
        self._step_dev = None            # use_device_step(): the step counter lives in device memory (graph-replayable)
        self._lib, self._ct = _lib, ctypes
        size = self.pc_pos.shape[0] if self.tri is None else self.tri.shape[0]
        if index == "auto":
            least = AUTO_TREE_MIN_POINTS if self.tri is None else AUTO_TREE_MIN_TRIANGLES
            index = "tree" if least is not None and size >= least else "brute"
        self.index = index
        self._mesh_index = self._cloud_index = None          # the BVH buffer (uint8), held for the sampler's lifetime
        if index == "tree":
            from . import hip_ops
            if self.tri is None:
                self._cloud_index = hip_ops.cloud_index_build(self.pc_pos)
            else:
                self._mesh_index = hip_ops.mesh_index_build(self.tri)

    def use_device_step(self):
        """Keep the step counter in DEVICE memory from now on (`dudf_sample_batch_at`; advanced on the stream after every
        batch): an iteration captured in a HIP graph then draws a NEW batch at every replay — the trainer calls `replayed()`
        per replayed batch to keep the host-side count in step.  The batches are bit-identical to the host-counter path."""
        self._step_dev = torch.full((1,), self._step, dtype=torch.int64, device=self.device)

    def replayed(self, n=1):
        self._step += n

    def n_local(self):
        sl = lambda m: m * (self.rank + 1) // self.world - m * self.rank // self.world   # noqa: E731
        return sl(self.samplesOnSurface), sl(self.n_far), sl(self.n_near)

    @property
    def n_on_surface(self):
        """Leading on-surface points of THIS rank's batch ([on | far | near]; train.py passes it to loss_s1 as a hint)."""
        return self.n_local()[0]

    def sample(self, step, stats=None):
        """(x (n,3), normals (n,3), sdf (n,)) device tensors for global step `step` (None: the device counter of
        `use_device_step`); n_on leading on-surface points.  stats (index "tree" only): int64 CUDA tensor of 1, the number of
        exact distance evaluations is ADDED to it."""
        ct, lib = self._ct, self._lib.load()
        n_on, n_far, n_near = self.n_local()
        n = n_on + n_far + n_near
        x = torch.empty(n, 3, dtype=torch.float32, device=self.device)
        nrm = torch.empty(n, 3, dtype=torch.float32, device=self.device)
        sdf = torch.empty(n, dtype=torch.float32, device=self.device)
        P = lambda t: ct.c_void_p(t.data_ptr())   # noqa: E731
        with torch.cuda.device(self.device):
            head = (P(self.tri) if self.tri is not None else None, self.tri.shape[0] if self.tri is not None else 0,
                    P(self.pc_pos), P(self.pc_nrm), self.pc_pos.shape[0], self.samplesOnSurface, self.n_far, self.n_near, self.seed)
            tail = (self.rank, self.world, P(x), P(nrm), P(sdf), ct.c_void_p(torch.cuda.current_stream().cuda_stream))
            if self.index == "tree":
                B = lambda t: (P(t), t.numel()) if t is not None else (None, 0)   # noqa: E731
                tail = (self.rank, self.world, *B(self._mesh_index), *B(self._cloud_index), *tail[2:5],
                        P(stats) if stats is not None else None, tail[5])
                if step is None:
                    rc = lib.dudf_sample_batch_indexed_at(*head, P(self._step_dev), *tail)
                else:
                    rc = lib.dudf_sample_batch_indexed(*head, step, *tail)
            elif stats is not None:
                raise self._lib.DudfError("PointCloud.sample: stats counts the evaluations of index='tree' only")
            elif step is None:
                rc = lib.dudf_sample_batch_at(*head, P(self._step_dev), *tail)
            else:
                rc = lib.dudf_sample_batch(*head, step, *tail)
        self._lib.check(rc, "dudf_sample_batch_indexed" if self.index == "tree" else "dudf_sample_batch")
        return x, nrm, sdf

    def __iter__(self):
        for _ in range(self.batchesPerEpoch):
            if self._step_dev is not None:
                x, nrm, sdf = self.sample(None)
                self._step_dev += 1
            else:
                x, nrm, sdf = self.sample(self._step)
            self._step += 1
            yield x[None], nrm[None], sdf[None, :, None]
