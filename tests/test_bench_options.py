# coding: utf-8
"""CPU: what bench.py does beyond timing the headline, and how it writes its outputs.  A plain run (no --full) runs no
per-kernel pass, no 8x512 block and no CPU baseline; --full runs them where they apply.  `dump_outputs` writes float32
.npy files under the given names, whole below the size limit and as the same seeded sample above it."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402

PLAIN = ["--gpus", "1", "--steps", "20", "--warmup", "5"]


def test_plain_run_does_only_the_headline():
    for world in (1, 2):
        plan = bench.extras(bench.parse_args(PLAIN), world)
        assert plan == {"profile_steps": 0, "config3": False, "config3_1m": False, "cpu_baseline": False}, (world, plan)
    # the --full sub-switches select nothing on their own
    plan = bench.extras(bench.parse_args(PLAIN + ["--no-cpu-baseline", "--no-config3-1m"]), 1)
    assert plan == {"profile_steps": 0, "config3": False, "config3_1m": False, "cpu_baseline": False}


def test_full_run_adds_every_block_where_it_applies():
    plan = bench.extras(bench.parse_args(PLAIN + ["--full"]), 1)
    assert plan == {"profile_steps": bench.PROFILE_STEPS, "config3": True, "config3_1m": True, "cpu_baseline": True}
    plan = bench.extras(bench.parse_args(PLAIN + ["--full"]), 8)                     # N ranks: no 1-GPU block, no CPU baseline
    assert plan == {"profile_steps": bench.PROFILE_STEPS, "config3": True, "config3_1m": False, "cpu_baseline": False}
    plan = bench.extras(bench.parse_args(PLAIN + ["--full", "--no-config3", "--no-cpu-baseline"]), 1)
    assert plan == {"profile_steps": bench.PROFILE_STEPS, "config3": False, "config3_1m": False, "cpu_baseline": False}
    plan = bench.extras(bench.parse_args(PLAIN + ["--full", "--no-config3-1m"]), 1)
    assert plan["config3"] and not plan["config3_1m"]
    plan = bench.extras(bench.parse_args(PLAIN + ["--full", "--hidden", "512"]), 1)  # the 8x512 blocks belong to the headline only
    assert plan["profile_steps"] and not plan["config3"] and not plan["config3_1m"] and plan["cpu_baseline"]


def test_dump_outputs_below_the_limit(tmp_path):
    rng = np.random.default_rng(1)
    arrays = {"loss_terms": rng.random(4).astype(np.float32), "theta": rng.random((10, 7)).astype(np.float32),
              "dtheta": rng.random(70)}                                              # float64 in: written as float32
    bench.dump_outputs(str(tmp_path), arrays)
    assert sorted(os.listdir(tmp_path)) == ["dtheta.npy", "loss_terms.npy", "theta.npy"]
    for name, a in arrays.items():
        got = np.load(tmp_path / f"{name}.npy")
        assert got.dtype == np.float32 and got.shape == a.shape and np.array_equal(got, a.astype(np.float32)), name


def test_dump_outputs_above_the_limit_is_the_same_seeded_sample(tmp_path):
    arrays = {"theta": np.arange(30000, dtype=np.float32), "dtheta": -np.arange(10000, dtype=np.float32)}
    limit = 40000                                                                    # bytes: a third of the 160 000 given
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays, limit=limit)
    total = 0
    for name, a in arrays.items():
        got = np.load(tmp_path / "a" / f"{name}.npy")
        assert got.dtype == np.float32 and got.ndim == 1
        assert got.size == a.size * limit // 160000                                  # each array its share of the limit
        assert np.array_equal(got, np.load(tmp_path / "b" / f"{name}.npy"))         # the same elements every time
        idx = np.abs(got).astype(np.int64)                                           # the values are their own indices here
        assert (np.diff(idx) > 0).all() and np.array_equal(got, a[idx])             # distinct elements, in index order
        total += got.nbytes
    assert total <= limit
