# coding: utf-8
"""GPU: the loss kernels alone (loss_fwd, loss_bwd, s2_stats, s2_terms of csrc/dudf_loss.hip, through dudf_debug_loss_stage) on the
planted inputs of tests/loss_stage_cases.py, against the oracle's loss_*_terms in float64 on the same float32 bits, POINT BY POINT —
no sweep in front, no adjoint sweep or weight-gradient GEMM behind, no max-norm over d(theta).  Every case runs with and without the
`deterministic` option.

  terms, stats   relative error against the oracle (terms: TOL_TERM = 1e-5, the suite's; the count exactly, the two sums 1e-12 of
                 sum |y| and sum y^2: fp64 sums of exact fp64 products); `deterministic`: two calls are bit-equal
  cotangents     per point: |got - ref| <= tol * max|ref over that point's ybar, gbar, Hbar| + 1.4e-45 — ybar and gbar under TOL_POINT,
                 Hbar (fp64 in the kernel, rounded once) under TOL_HBAR; the worst point is reported by case and class
  exact          the exact-kink cotangents are 0, loss_s2's off-surface ybar is 0, no padded column and no tangent-channel ybar holds
                 anything but +0 (NaN cases included), the cos == 0 point contributes exactly 1 and has Hbar == 0, the Hessian's upper
                 triangle changes no bit and Hbar is symmetric in all nine entries
  non-finite     a degenerate top gap gives an all-non-finite Hbar, one or identical on-surface points of loss_s2 a non-finite ybar
                 — there and in the oracle — and every other point is bit-equal to the same batch with that point made generic; a
                 Hessian-path point off the surface gives four NaN terms and a NaN ybar at that point alone

TOLERANCES.  Not fixed in advance: four times the worst per-point figure measured on an MI355X over all finite cases, rounded up to one
significant digit, and never above 1e-5 (the suite's bar on the terms).  Measured (MEASURED below):
    ybar, gbar   3.78e-7 (loss_siren, zero normal: 2 (|g| - 1) / |g| in fp32 at |g| = 1.25)   -> TOL_POINT = 2e-6
    Hbar         6.19e-8 (loss_s1, a generic Hessian: fp64 rounded once)                       -> TOL_HBAR  = 3e-7
    terms        1.62e-6 (loss_s1 off-surface term of 3 points, each 2 % beside its kink)      (TOL_TERM  = 1e-5)
    worst by mode: loss_s1 ybar/gbar 1.4e-7, Hbar 6.2e-8; loss_siren 3.8e-7; loss_s2 at most 9.1e-8.  tanhf(50) is exactly 1 on the device
    (the exact-kink cotangents are 0), a float32 denormal y keeps its sign, expf(-100) gives a denormal ybar within one step.
FOUND by these cases and fixed in csrc/dudf_loss.hip: loss_siren's alignment cotangent k1 m - k2 g was formed in fp32, where it cancels
for g parallel to the normal — 1.6e-5 (g || +m) and 4.4e-6 (g || -m) of the point's largest cotangent, above any bound this test may
set; it is formed in fp64 now (3.1e-7, what the fp32 Eikonal part next to it leaves).  s2_terms reported a std of 0 for fewer than
two on-surface points where torch.std (reference src/loss_functions.py:115) and the oracle give NaN."""
import numpy as np
import pytest
import torch

import loss_stage_cases as C

pytestmark = pytest.mark.gpu

# measured on an MI355X (worst per-point relative error over all finite cases) -> 4 x, rounded up to one significant digit
MEASURED = {"point": 3.78e-7, "hbar": 6.19e-8, "terms": 1.62e-6}
TOL_POINT = 2e-6
TOL_HBAR = 3e-7
TOL_TERM = 1e-5
DENORM = 1.4e-45
HIDDEN = [32, 32]                                           # the loss stage never looks at the network: the smallest workspace

CASES = C.all_cases()
IDS = [c["name"] for c in CASES]
MODES = {"s1": 0, "s2": 1, "siren": 2}


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible")
    from diffudf_amd import hip_ops
    return hip_ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(hip, c, deterministic=0, h=None):
    """the case on the device -> numpy dict (terms, stats, ybar, gbar, hbar, pad_nonzero); one workspace per (n, n_hess)"""
    cfg = hip.make_cfg(HIDDEN)
    ws = hip.workspace_for(cfg, c["n"], "cuda", n_hess=c["n_hess"])
    hh = c["h"] if h is None else h
    with hip.options(deterministic=deterministic):
        out = hip.debug_loss_stage(cfg, MODES[c["mode"]], dev(c["y"]), dev(c["g"]), dev(hh) if c["n_hess"] else None, dev(c["normals"]),
                                   dev(c["sdf"]), c["n_global"], c["weights"], c["alpha"], dev(np.asarray(c["cot"], dtype=np.float32)), ws,
                                   stats=None if c["stats"] is None else dev(c["stats"]))
    torch.cuda.synchronize()
    res = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}
    if res["hbar"] is None:
        res["hbar"] = np.zeros((0, 3, 3), np.float32)
    return res


@pytest.fixture(scope="module")
def results(hip):
    """every case (and twin) once per setting of `deterministic`, and the oracle's answer once"""
    out = {}
    for c in CASES:
        out[c["name"]] = {"ref": C.reference(c), 0: run(hip, c, 0), 1: run(hip, c, 1), "again": run(hip, c, 1)}
        if c["twin"] is not None:
            out[c["name"]]["twin"] = {0: run(hip, c["twin"], 0), 1: run(hip, c["twin"], 1)}
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def finite_points(c):
    ok = np.ones(c["n"], bool)
    ok[c["nonfinite"]] = False
    ok[c["poison"]] = False
    return ok


def point_errors(c, got, ref):
    """per point: (error of ybar and gbar, error of Hbar (0 behind n_hess), the point's scale max|ref|)"""
    n, nh = c["n"], c["n_hess"]
    scale = np.maximum(np.abs(ref["ybar"]), np.abs(ref["gbar"]).max(1))
    e_h = np.zeros(n)
    if nh:
        with np.errstate(invalid="ignore"):
            scale[:nh] = np.maximum(scale[:nh], np.abs(ref["hbar"]).max((1, 2)))
            e_h[:nh] = np.abs(got["hbar"].astype(np.float64) - ref["hbar"]).max((1, 2))
    e_p = np.maximum(np.abs(got["ybar"].astype(np.float64) - ref["ybar"]), np.abs(got["gbar"].astype(np.float64) - ref["gbar"]).max(1))
    return e_p, e_h, scale


def test_the_inputs_keep_their_margin():
    for c in CASES:
        dist, kink, p = C.margin(c)
        assert dist >= C.MARGIN, (c["name"], kink, p, dist)


def test_terms_and_stats(results, capsys):
    worst = (0.0, "")
    for c in CASES:
        r = results[c["name"]]
        for det in (0, 1):
            got, ref = r[det], r["ref"]
            if c["poison"]:
                assert np.isnan(got["terms"]).all(), (c["name"], got["terms"])
                continue
            for i in range(4):
                if i in c["skip_terms"]:                    # a degenerate top eigenvector is any vector of a plane: no reference value
                    assert np.isfinite(got["terms"][i])
                    continue
                want = ref["terms"][i]
                if not np.isfinite(want):
                    assert np.isnan(got["terms"][i]) == np.isnan(want), (c["name"], i, got["terms"], ref["terms"])
                elif want == 0:
                    assert got["terms"][i] == 0, (c["name"], i, got["terms"])
                else:
                    rel = abs(float(got["terms"][i]) - want) / abs(want)
                    worst = max(worst, (rel, f"{c['name']} term {i}"))
                    assert rel <= TOL_TERM, (c["name"], i, got["terms"], ref["terms"], rel)
            if c["mode"] == "s2":
                y64 = c["y"].astype(np.float64)[c["sdf"] == 0]
                assert got["stats"][0] == ref["stats"][0] == y64.size
                assert abs(got["stats"][1] - ref["stats"][1]) <= 1e-12 * max(np.abs(y64).sum(), 1e-300) or y64.size == 0
                assert abs(got["stats"][2] - ref["stats"][2]) <= 1e-12 * max((y64 * y64).sum(), 1e-300) or y64.size == 0
        if "identical" in c["name"]:
            assert r[0]["terms"][1] == 0 and r[1]["terms"][1] == 0
    with capsys.disabled():
        print(f"\n  loss stage terms: worst relative error {worst[0]:.2e} ({worst[1]})", end="")


def test_cotangents_point_by_point(results, capsys):
    worst_p, worst_h, by_class, failures = (0.0, ""), (0.0, ""), {}, []
    for c in CASES:
        ok = finite_points(c)
        for det in (0, 1):
            got, ref = results[c["name"]][det], results[c["name"]]["ref"]
            e_p, e_h, scale = point_errors(c, got, ref)
            # cos = +-1: Hbar is rounding noise of the eigenvector (450 eps, tests/test_eigh3_gpu.py) over a gap >= 1, times the factor
            k2 = abs(c["weights"][2] * c["cot"][2]) / c["n_global"] if c["mode"] == "s1" else 0.0
            allow_h = np.where(c["parallel"], 1e-13 * k2, 0.0)
            for p in np.nonzero(ok)[0]:
                assert np.isfinite(got["ybar"][p]) and np.isfinite(got["gbar"][p]).all(), (c["name"], p, c["kind"][p])
                assert p >= c["n_hess"] or np.isfinite(got["hbar"][p]).all(), (c["name"], p, c["kind"][p])
                rp = e_p[p] / scale[p] if scale[p] > 0 else 0.0
                rh = max(e_h[p] - allow_h[p], 0.0) / scale[p] if scale[p] > 0 else 0.0
                label = f"{c['name']} point {p} ({c['kind'][p]})"
                worst_p, worst_h = max(worst_p, (rp, label)), max(worst_h, (rh, label))
                for cls in c["kind"][p].split(" "):
                    a = by_class.setdefault(cls, [0.0, 0.0])
                    a[0], a[1] = max(a[0], rp), max(a[1], rh)
                if e_p[p] > TOL_POINT * scale[p] + DENORM:
                    failures.append(("ybar/gbar", label, e_p[p], scale[p]))
                if e_h[p] > TOL_HBAR * scale[p] + allow_h[p] + DENORM:
                    failures.append(("Hbar", label, e_h[p], scale[p]))
    with capsys.disabled():
        print(f"\n  loss stage per point: ybar/gbar worst {worst_p[0]:.2e} at {worst_p[1]}\n"
              f"  loss stage per point: Hbar worst {worst_h[0]:.2e} at {worst_h[1]}", end="")
        for cls in sorted(by_class):
            print(f"\n    class {cls:28s} ybar/gbar {by_class[cls][0]:.2e}  Hbar {by_class[cls][1]:.2e}", end="")
    assert not failures, failures[:10]


def test_exact_statements(results):
    for c in CASES:
        n, nh = c["n"], c["n_hess"]
        for det in (0, 1):
            got = results[c["name"]][det]
            assert got["pad_nonzero"] == 0, (c["name"], det)
            if "twin" in results[c["name"]]:
                assert results[c["name"]]["twin"][det]["pad_nonzero"] == 0
            if c["mode"] == "s2":
                assert (bits(got["ybar"][c["sdf"] != 0]) == 0).all() and (bits(got["gbar"]) == 0).all(), c["name"]
                continue
            ok = finite_points(c)
            assert (got["ybar"][c["exact"]["y"] & ok] == 0).all(), c["name"]
            if c["mode"] == "s1":
                assert (got["gbar"][c["exact"]["g"]] == 0).all(), c["name"]
                g64 = c["g"].astype(np.float64)
                assert (got["gbar"][(g64 * g64).sum(-1) == 0] == 0).all(), c["name"]
            if nh and c["weights"][2] != 0:
                cs0 = c["exact"]["cs"][:nh] & ~c["exact"]["gap"][:nh]
                assert (got["hbar"][cs0] == 0).all(), c["name"]
                fin = ok[:nh]
                assert (bits(got["hbar"][fin]) == bits(np.transpose(got["hbar"][fin], (0, 2, 1)))).all(), c["name"]   # all nine entries


def test_the_cos_zero_point_contributes_exactly_one(hip):
    """the point alone, with w / N = 1: its term is the whole sum"""
    one = C.s1_case("cs0 alone", 1, 1, [1.0, 1.0, 1.0, 0.0], 100.0, C.COT_ONES)
    one["h"][0], one["normals"][0], one["y"][0] = np.diag([1.0, 2.0, 3.0]), [1.0, 0.0, 0.0], 0.25
    for m in ([1.0, 0.0, 0.0], [0.0, -3.0, 0.0], [0.0, 0.0, 0.0]):       # orthogonal to e_z twice, and the clamped zero normal
        one["normals"][0] = m
        got = run(hip, one)
        assert got["terms"][2] == 1.0 and got["terms"][0] == 0.25 and (got["hbar"] == 0).all() and got["pad_nonzero"] == 0, (m, got)


def test_the_upper_triangle_changes_no_bit(hip, results):
    for c in CASES:
        if not (c["upper"].any() and not c["poison"]):
            continue
        sym = np.tril(c["h"]) + np.transpose(np.tril(c["h"], -1), (0, 2, 1))
        assert (sym != c["h"]).any()
        for det in (0, 1):
            a, b = results[c["name"]][det], run(hip, c, det, h=sym)
            for k in ("ybar", "gbar", "hbar"):
                assert (bits(a[k]) == bits(b[k])).all(), (c["name"], k)
            if det:
                assert (bits(a["terms"]) == bits(b["terms"])).all(), c["name"]


def test_deterministic_calls_are_bit_equal(results):
    for c in CASES:
        a, b = results[c["name"]][1], results[c["name"]]["again"]
        for k in ("terms", "ybar", "gbar", "hbar") + (("stats",) if c["mode"] == "s2" else ()):
            assert (bits(a[k]) == bits(b[k])).all(), (c["name"], k)
        if c["mode"] == "s2":                               # its cotangents read the statistics, whose last bit is the summation order's
            continue
        a0 = results[c["name"]][0]                          # loss_s1, loss_siren: the cotangents are per point, whatever the grid
        for k in ("ybar", "gbar", "hbar"):
            assert (bits(a[k]) == bits(a0[k])).all(), (c["name"], k)


def test_non_finite_outcomes_match_the_oracle_and_stay_local(results):
    seen = set()
    for c in CASES:
        if c["twin"] is None:
            continue
        ref = results[c["name"]]["ref"]
        ok = finite_points(c)
        for det in (0, 1):
            got, twin = results[c["name"]][det], results[c["name"]]["twin"][det]
            for p in c["nonfinite"]:
                if c["mode"] == "s1":
                    assert not np.isfinite(got["hbar"][p]).any() and not np.isfinite(ref["hbar"][p]).any(), (c["name"], p)
                    assert np.isfinite(got["ybar"][p]) and np.isfinite(got["gbar"][p]).all()
                    seen.add("degenerate")
                else:
                    assert not np.isfinite(got["ybar"][p]) and not np.isfinite(ref["ybar"][p]), (c["name"], p)
                    seen.add("s2")
            for p in c["poison"]:
                assert np.isnan(got["ybar"][p]) and np.isnan(got["terms"]).all(), (c["name"], p)
                seen.add("poison")
            for k in ("ybar", "gbar"):
                assert (bits(got[k][ok]) == bits(twin[k][ok])).all(), (c["name"], k)
            okh = ok[: c["n_hess"]]
            assert (bits(got["hbar"][okh]) == bits(twin["hbar"][okh])).all(), c["name"]
    assert seen == {"degenerate", "s2", "poison"}
