# coding: utf-8
"""GPU: edge shapes through the training path in every stash format (tools/stress_modes.py): 13 networks — one / 17 / skewed-stride
column counts, all-quad batches, 2 ... 34 hidden layers, 256 and 512 wide, `loss_s1` with and without the Hessian term and
`loss_s2` — must give the same terms and d(theta) with the fp32 stash (option stash = 0), R, E, C at 24 bits (6) and the default:
all seven arrays at 24 bits (7).  The formats are switched in-process through dudf_set_option.
(HIP against HIP, over the whole d(theta): a defect all three formats share passes here.  The oracle comparisons of the edge column
counts, per parameter tensor, are in test_dtheta_edges_gpu.py; this file adds the deep networks and the skewed row stride, which
cost the oracle too much.)"""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(REPO, "tools", "stress_modes.py")


def test_edge_shapes_agree_across_stash_formats(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("stress_modes", TOOL)
    sm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sm)
    outs = {}
    for tag, stash in (("fp32", 0), ("rec24", 6), ("all24", 7)):
        outs[tag] = str(tmp_path / f"{tag}.npz")
        modes = sm.run(outs[tag], stash)
        assert modes <= {stash, 0, 6}, (tag, modes)          # (deep / 512-wide cases fall back)
        assert stash in modes, (tag, modes)
    for other in ("rec24", "all24"):
        sm.compare(outs["fp32"], outs[other])
