# coding: utf-8
"""Dense oriented point cloud from a trained network — reference src/render_pc.py:10-73 (`Sampler`), same names, signatures
and return types.  The reference's round is host-bound (per step two `evaluate` calls in chunks of 64^2 with a D2H copy each,
numpy masking, one `np.linalg.eigh` per accepted point); here the samples, the growing surface buffer and the normals stay in
device memory and a round is a fixed short chain of kernels (csrc/dudf_pointcloud.hip, dudf_pointcloud_round)."""
import os
import warnings

import numpy as np
import torch

from . import hip_ops
from ._lib import DudfError
from .model import SIREN


class Sampler:
    def __init__(self, n_in_features=3, hidden_layers=[256, 256, 256, 256], w0=30, ww=None, checkpoint=None, device=0):
        """reference src/render_pc.py:11-24"""
        self.decoder = SIREN(n_in_features=n_in_features, n_out_features=1, hidden_layer_config=hidden_layers, w0=w0, ww=ww)
        self.features = n_in_features
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self.decoder.to(self.device)
        self.decoder.eval()
        self.decoder.load_state_dict(torch.load(checkpoint, map_location=self.device, weights_only=True))

    @classmethod
    def from_model(cls, model):
        """A Sampler around a `SIREN` the caller already holds (no checkpoint file)."""
        self = cls.__new__(cls)
        self.decoder = model
        self.features = model.n_in_features
        self.device = model.flat_parameters().device
        self.decoder.eval()
        return self

    def generate_point_cloud(self, gt_mode, alpha, num_steps=5, num_points=20000, surf_thresh=0.01, max_iter=1000, *,
                             rng="numpy", seed=None, check_every=8, return_tensors=False):
        """reference src/render_pc.py:26-73: (surface_points (m,3), normals (m,3)) float64 numpy arrays, m >= num_points unless
        `max_iter` rounds did not find that many (RuntimeWarning, as there).

        rng="numpy" (default): the proposals' random numbers are drawn on the host with `np.random` in the reference's call order
        and shapes — a seeded run consumes the same stream as the reference — and uploaded, one buffer per round.
        rng="device": a counter-based generator inside the propose kernel, a pure function of (seed, round, row); the row count is
        then read back only every `check_every` rounds where the round does not need it itself (rounds issued after the quota is
        reached change nothing).  seed: `np.random.seed(seed)` / the device generator's key; None = leave numpy's state alone /
        a fresh key.  return_tensors: float64 CUDA tensors instead of numpy arrays."""
        if rng not in ("numpy", "device"):
            raise ValueError(f"rng must be 'numpy' or 'device'; got {rng!r}")
        if gt_mode not in hip_ops.INVERSE_MODES:
            raise KeyError(gt_mode)
        num_points, num_steps, check_every = int(num_points), int(num_steps), max(int(check_every), 1)
        theta = self.decoder.flat_parameters()
        if theta.device.type != "cuda":
            raise DudfError(f"Sampler: the network must live on the GPU (got {theta.device}); the HIP path has no CPU fallback")
        for param in self.decoder.parameters():
            param.requires_grad = False
        cfg, dev = self.decoder.hip_cfg, theta.device
        if rng == "numpy" and seed is not None:
            np.random.seed(seed)
        if rng == "device" and seed is None:
            seed = int.from_bytes(os.urandom(8), "little")
        state = hip_ops.PointCloudState(cfg, num_points, dev)
        half, held = num_points // 2, 0
        for iteration in range(max_iter):
            if rng == "numpy":
                if held != 0:       # :36-37, in the reference's order: indices, noise, uniforms
                    idx = np.random.uniform(0, held, half).astype(np.uint32)
                    noise = np.random.normal(0, 0.1, (half, 3))
                    uni = np.random.uniform(-1, 1, (half, 3))
                    buf = np.concatenate([idx.astype(np.float64), noise.reshape(-1), uni.reshape(-1)])
                else:               # :39
                    buf = np.random.uniform(-1, 1, (num_points, 3)).reshape(-1)
                rand = torch.from_numpy(np.ascontiguousarray(buf)).to(dev) if buf.size else None
                held = hip_ops.pointcloud_round(cfg, theta, state, gt_mode, alpha, num_steps, surf_thresh, rand=rand)[0]
            else:
                # the Hessian normals need the accepted count on the host anyway; 'siren' rounds only enqueue
                want = gt_mode != "siren" or (iteration + 1) % check_every == 0 or iteration + 1 == max_iter
                c = hip_ops.pointcloud_round(cfg, theta, state, gt_mode, alpha, num_steps, surf_thresh, rand=None, seed=seed,
                                             want_count=want)
                if c is not None:
                    held = c[0]
            if held >= num_points:      # :67
                break
        held = state.count()
        if held < num_points:
            warnings.warn('\033[93m' + f'Max iterations reached. Only sampled {held} surface points.' + '\033[0m', RuntimeWarning)
        points, normals = state.points[:held], state.normals[:held]
        if return_tensors:
            return points.clone(), normals.clone()
        return points.cpu().numpy(), normals.cpu().numpy()
