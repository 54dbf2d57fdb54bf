# coding: utf-8
"""CPU: the per-tensor and per-band error measures of tests/parity_util.py see what the max-norm over the flat d(theta) does not.
An oracle gradient of the 8x256 network (loss_s2, 1000 points) with the first layer's db, or one band of 16 rows of a hidden dW,
off by 0.5 % stays under the 1e-4 bar of the flat vector — the first layer's gradients are 1.5e-2 of the largest entry there, that
band 1.2e-2 — and is flagged, by name, by `per_tensor_rel` and `per_band_rel`."""
import numpy as np

import parity_util as U

HIDDEN, N, SEED, LOSS = (256,) * 8, 1000, 123, "s2"


def case():
    P, _ = U.net(HIDDEN, SEED)
    _, grads, _ = U.thirds_case(HIDDEN, N, SEED, LOSS)
    return P, grads


def test_exact_gradient_has_no_error_and_no_skipped_band():
    P, grads = case()
    assert max(e for _, e in U.per_tensor_rel(U.flat(grads), grads, P)) == 0.0
    name, band, skipped = U.worst_band(U.flat(grads), grads, P)
    assert band.err == 0.0 and skipped == 0 and band.bands == 2 * 256 // 16
    assert [n for n, _, _, _ in U.tensor_slices(P)][:4] == ["dW0", "db0", "dW1", "db1"]


def test_first_layer_bias_off_by_half_a_percent_is_flagged():
    P, grads = case()
    bad = [(w.copy(), b.copy()) for w, b in grads]
    bad[0][1][:] *= 1.005
    assert U.rel(U.flat(bad), U.flat(grads)) < U.TOL_DTHETA[LOSS]          # the flat max-norm lets it through
    per = dict(U.per_tensor_rel(U.flat(bad), grads, P))
    assert [n for n, e in per.items() if e >= U.TOL_DTHETA[LOSS]] == ["db0"] and abs(per["db0"] - 0.005) < 1e-6
    band = U.per_band_rel(bad[0][1], grads[0][1])
    assert band.err > U.BAND_TOL and abs(band.err - 0.005) < 1e-6 and band.axis == "rows" and band.skipped == 0


def test_one_band_of_a_hidden_matrix_off_by_half_a_percent_is_flagged_by_name():
    P, grads = case()
    bad = [(w.copy(), b.copy()) for w, b in grads]
    bad[1][0][144:160] *= 1.005
    assert U.rel(U.flat(bad), U.flat(grads)) < U.TOL_DTHETA[LOSS]
    per = dict(U.per_tensor_rel(U.flat(bad), grads, P))
    assert [n for n, e in per.items() if e >= U.TOL_DTHETA[LOSS]] == ["dW1"]
    name, band, skipped = U.worst_band(U.flat(bad), grads, P)
    assert (name, band.axis, band.index, skipped) == ("dW1", "rows", 9, 0)
    assert band.err > U.BAND_TOL and abs(band.err - 0.005) < 1e-6 and str(band).startswith("rows 144..159")


def test_padded_layout_round_trip_and_zero_bands():
    """pad_theta / unpad_flat are inverse on the caller's entries; a band whose reference is all zero is skipped and counted"""
    P, _ = U.net((200,) * 3, 6)
    th = U.pad_theta(P, 256)
    assert th.size == 4 * 256 + 2 * (256 * 256 + 256) + 257 and np.array_equal(U.unpad_flat(th, P, 256), U.flat(P))
    ref = np.ones((32, 32)); ref[16:] = 0.0
    band = U.per_band_rel(ref, ref)
    assert band.skipped == 1 and band.bands == 3 and band.err == 0.0


def test_launch_geometry_restated():
    assert U.wgrad_columns(1) == 128 and U.wgrad_columns(129) == 256 and U.wgrad_columns(100, 32) == 256 and U.wgrad_columns(100, 33) == 384
    assert U.wgrad_nsplit(256, 3, 700, 0, cap=8) == (4, 24, 2) and U.wgrad_nsplit(256, 8, 1000, 0, cap=8) == (1, 32, 7)
    assert U.wgrad_nsplit(256, 2, 17) == (4, 4, 1) and U.wgrad_nsplit(512, 2, 129)[0] == 8 and U.wgrad_nsplit(256, 3, 700, deterministic=1)[0] == 1
