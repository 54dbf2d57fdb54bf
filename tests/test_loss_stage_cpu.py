# coding: utf-8
"""CPU: the planted inputs of the loss stage (tests/loss_stage_cases.py) are what they claim to be, and the oracle the GPU test
(tests/test_loss_stage_gpu.py) trusts is pinned AT those points.

  * every non-exact point keeps a relative distance of at least 1e-4 to its nearest kink under the oracle's fp64 evaluation (100 % of
    them: nothing is replaced), arrays have the stated shapes, are float32 and obey the magnitude rule;
  * the closed-form cotangents of `loss_s1_terms` / `loss_siren_terms` / `loss_s2_terms` equal torch.autograd's of the sum of the terms
    (float64, the Hessian's symmetrised) within 1e-10 of each point's largest cotangent, at every point that is neither an exact
    kink, nor inside a clamp, nor non-finite (measured on a CPU: 6.2e-16 worst over these cases, 1e-14 on a random
    batch);
  * where autograd has no say (sqrt at 0 is NaN, abs at 0 is a choice) the literal convention is asserted instead: sign(0) = 0, a
    zero gradient of the norm at 0, a constant norm factor inside the 1e-8 clamp of the cosine."""
import numpy as np
import pytest
import torch

import loss_stage_cases as C
from oracle import dudf_oracle as O

CASES = C.all_cases()
IDS = [c["name"] for c in CASES]
REFS = {}


def ref_of(c):
    if c["name"] not in REFS:
        REFS[c["name"]] = C.reference(c)
    return REFS[c["name"]]


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_every_point_keeps_its_margin(c):
    dist, kink, p = C.margin(c, ref_of(c))
    assert dist >= C.MARGIN, (c["name"], kink, p, c["kind"][p] if p >= 0 else "", dist)
    if c["twin"] is not None:
        dist, kink, p = C.margin(c["twin"])
        assert dist >= C.MARGIN, (c["twin"]["name"], kink, p, dist)


def test_case_names_are_unique_and_the_shapes_are_the_stated_ones():
    assert len(set(IDS)) == len(IDS)
    s1 = {(c["n"], c["n_hess"]) for c in CASES if c["mode"] == "s1"}
    assert set(C.SHAPES) <= s1
    assert any(c["n_global"] == 3 * c["n"] for c in CASES if c["mode"] == "s1")
    for mode, ws in (("s1", (C.W_EIK, C.W_HESS, C.W_HESS_ONLY)), ("siren", (C.W_SIREN,)), ("s2", (C.W_S2,))):
        assert {tuple(c["weights"]) for c in CASES if c["mode"] == mode} == {tuple(w) for w in ws}
    assert {c["alpha"] for c in CASES if c["mode"] == "s1"} == {100.0, 10.0}
    assert {tuple(c["cot"]) for c in CASES if c["mode"] != "s2"} == {tuple(C.COT_ONES), tuple(C.COT_MIXED)}


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_arrays_are_float32_of_the_stated_shapes_and_magnitudes(c):
    n, nh = c["n"], c["n_hess"]
    for k, shape in (("y", (n,)), ("g", (n, 3)), ("h", (nh, 3, 3)), ("normals", (n, 3)), ("sdf", (n,))):
        assert c[k].dtype == np.float32 and c[k].shape == shape and np.isfinite(c[k]).all(), (c["name"], k)
    assert len(c["kind"]) == n and all(c["kind"])
    for k in ("g", "normals"):
        nrm = np.sqrt((c[k].astype(np.float64) ** 2).sum(-1))
        assert ((nrm == 0) | ((nrm >= 0.99e-15) & (nrm <= 1.01e15))).all(), (c["name"], k)
        sq = c[k] * c[k]                                    # the fp32 squares: no underflow to 0 or to a denormal, no overflow
        assert ((c[k] == 0) | (sq >= np.finfo(np.float32).tiny)).all() and np.isfinite(sq).all(), (c["name"], k)
    if c["mode"] == "s1" and c["weights"][2] != 0 and not c["poison"]:
        assert ((np.arange(n) < nh) == (c["sdf"] == 0)).all()


def smooth_mask(c):
    """points where the loss is differentiable and finite: autograd and the closed form must agree there"""
    g = c["g"].astype(np.float64)
    bad = c["exact"]["y"] | c["exact"]["g"] | c["exact"]["cs"] | c["exact"]["gap"] | c["parallel"] | c["clamp"] | ((g * g).sum(-1) == 0)
    bad[c["nonfinite"]] = True
    bad[c["poison"]] = True
    return ~bad


AUTOGRAD = [c for c in CASES if not c["poison"] and (c["mode"] != "s2" or (c["stats"] is None and not c["nonfinite"] and not c["exact_mu"]))]


@pytest.mark.parametrize("c", AUTOGRAD, ids=[c["name"] for c in AUTOGRAD])
def test_closed_form_cotangents_are_autograd_of_the_terms(c, capsys):
    y, g, H, m, sdf = (torch.from_numpy(a) for a in C.oracle_inputs(c))
    wc = [float(a * b) for a, b in zip(c["weights"], c["cot"])]
    for t in (y, g, H):
        t.requires_grad_(True)
    if c["mode"] == "s1":
        terms, cot = O.loss_s1_terms(y, g, H, m, sdf, wc, c["alpha"], xp=torch)
    elif c["mode"] == "siren":
        terms, cot = O.loss_siren_terms(y, g, m, sdf, wc, xp=torch)
    else:
        terms, cot = O.loss_s2_terms(y, sdf, wc, xp=torch)
    total = sum(t for t in terms.values() if torch.is_tensor(t) and t.requires_grad)
    ay, ag, aH = torch.autograd.grad(total, [y, g, H], allow_unused=True)
    n, nh = c["n"], c["n_hess"]
    zeros = lambda t, like: torch.zeros_like(like) if t is None else t.detach()  # noqa: E731
    ay, ag, aH = zeros(ay, y), zeros(ag, g), zeros(aH, H)
    aH = 0.5 * (aH + aH.transpose(1, 2))
    cy = cot["ybar"].detach()
    cg = zeros(cot.get("gbar"), g)
    cH = zeros(cot.get("Hbar"), H)
    ok = torch.from_numpy(smooth_mask(c))
    assert ok.any() or n <= 5 or c["mode"] == "s2"
    scale = torch.maximum(torch.maximum(cy.abs(), cg.abs().amax(1)), cH.abs().amax((1, 2)))
    err = torch.maximum(torch.maximum((ay - cy).abs(), (ag - cg).abs().amax(1)), (aH - cH).abs().amax((1, 2)))
    rel = torch.where(ok & (scale > 0), err / scale.clamp_min(1e-300), torch.zeros_like(err))
    if c["mode"] == "s2":                                   # one coupled sum: every on-surface point is smooth or none is
        rel = err / scale.max().clamp_min(1e-300)
    worst = int(rel.argmax())
    with capsys.disabled():
        print(f"\n  autograd vs closed form, {c['name']}: worst {float(rel.max()):.2e} at point {worst} ({c['kind'][worst]})", end="")
    assert torch.isfinite(rel).all() and float(rel.max()) <= 1e-10, (c["name"], worst, c["kind"][worst])
    assert (err[ok & (scale == 0)] == 0).all()
    assert (aH[nh:] == 0).all() and (cH[nh:] == 0).all()    # a point without a Hessian has no Hessian cotangent


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_literal_conventions_at_kinks_clamps_and_non_finite_points(c):
    r = ref_of(c)
    n, nh = c["n"], c["n_hess"]
    g64, m64 = c["g"].astype(np.float64), c["normals"].astype(np.float64)
    gn, mn = np.sqrt((g64 * g64).sum(-1)), np.sqrt((m64 * m64).sum(-1))
    wc = np.asarray(c["weights"], dtype=np.float64) * np.asarray(c["cot"], dtype=np.float64)[: len(c["weights"])]
    N = c["n_global"]
    fin = np.ones(n, bool)
    fin[c["nonfinite"]] = False
    if c["mode"] == "s1":
        assert (r["ybar"][c["exact"]["y"]] == 0).all()                       # sign(0) = 0
        assert (r["gbar"][c["exact"]["g"]] == 0).all()
        assert (r["gbar"][gn == 0] == 0).all()                                # the norm's gradient at 0 is 0, not sqrt's NaN
        cs0 = c["exact"]["cs"][:nh] & ~c["exact"]["gap"][:nh]
        if c["weights"][2] != 0 and nh:
            assert (r["cos"][:nh][cs0] == 0).all() and (r["hbar"][cs0] == 0).all()
            par = c["parallel"][:nh]
            assert (np.abs(np.abs(r["cos"][:nh][par]) - 1) <= 1e-15).all()
            assert (np.abs(r["hbar"][par]) <= 1e-13 * wc[2] / N).all()        # gaps of these matrices are >= 1
            for p in c["nonfinite"]:
                assert not np.isfinite(r["hbar"][p]).any(), (c["name"], p)
            assert np.isfinite(r["hbar"][fin[:nh]]).all()
        assert np.isfinite(r["ybar"]).all() and np.isfinite(r["gbar"]).all()
    elif c["mode"] == "siren":
        on = c["sdf"] == 0
        assert (r["ybar"][c["exact"]["y"]] == 0).all()
        eik = np.where(gn > 0, (wc[3] / N) * 2.0 * (gn - 1.0) / np.where(gn > 0, gn, 1.0), 0.0)[:, None] * g64
        inside = on & (gn <= 1e-8)                                            # the cosine's |g| is the constant 1e-8 there
        want = eik - (wc[2] / N) * m64 / (1e-8 * np.maximum(mn, 1e-8))[:, None]
        assert inside.sum() >= 2 or n < 8
        np.testing.assert_allclose(r["gbar"][inside], want[inside], rtol=1e-12, atol=0)
        zero_m = on & (mn == 0)
        np.testing.assert_allclose(r["gbar"][zero_m], eik[zero_m], rtol=1e-12, atol=0)
        assert np.isfinite(r["ybar"]).all() and np.isfinite(r["gbar"]).all()
    else:
        on = c["sdf"] == 0
        assert (r["ybar"][~on] == 0).all() and (r["gbar"] == 0).all()
        if c["nonfinite"]:
            assert not np.isfinite(r["ybar"][c["nonfinite"]]).any()
        if "identical" in c["name"]:
            assert r["terms"][1] == 0 and r["terms"][0] == 0.25 * c["weights"][0]
        if "one on-surface" in c["name"] or "no on-surface" in c["name"]:
            assert np.isnan(r["terms"][1])                                    # torch.std of one value, or of none (reference :115)
        if "no on-surface" in c["name"]:
            assert np.isnan(r["terms"][0])
        if "mu=0" in c["name"]:
            yo = c["y"][on].astype(np.float64)
            assert yo.sum() == 0 and r["terms"][0] == 0                       # sign(mu) = 0: only the std term has a cotangent
            sd = np.sqrt((yo * yo).sum() / (yo.size - 1))
            np.testing.assert_allclose(r["ybar"][on], wc[1] * yo / ((yo.size - 1) * sd), rtol=1e-12)
