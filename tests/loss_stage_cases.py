# coding: utf-8
"""Planted inputs of the loss stage and of the 3x3 eigensolver, shared by tests/test_loss_stage_cpu.py, tests/test_loss_stage_gpu.py and
tests/test_eigh3_gpu.py: named cases of (y, df/dx, Hessian, normals, sdf) that put every branch of the per-point loss code
(csrc/dudf_loss.hip) at a place of our choosing, the fp64 oracle's answer to each, and the distance of every point to its nearest kink.

Every value is float32-representable: the kernels load float32, the oracle gets the same bits as float64.

MAGNITUDES.  A vector (df/dx, a normal) has norm exactly 0 or within [1e-15, 1e15]: the fp32 squares in the kernels' |g| then neither
underflow nor overflow.  A vector whose squares underflow has |g| = 0 in the kernel and in a fp32 run of the reference, not in a fp64
oracle: that is a property of fp32, not a finding, so such vectors are not planted.

KINKS.  The loss is a sum of absolute values; a point sits on a kink where tdf - y, |g| - tau, cos, lam_2 - lam_j or the on-surface mean
mu is zero.  Points planted exactly ON a kink (y = 0 on the surface, u = y = 0.5 at alpha = 100, g = (0, 0, -1) there, a normal
orthogonal to the top eigenvector, a zero normal, mu = 0) are flagged per kink in `exact`; `margin(case)` is the smallest relative
distance of every other (point, kink) pair, and the tests hold it above MARGIN.  No point is ever replaced."""
import itertools

import numpy as np

from oracle import dudf_oracle as O

F32 = np.float32
FLT_MIN = float(np.finfo(F32).tiny)
DENORM = float(np.nextafter(F32(0), F32(1)))               # 1.4e-45, one float32 denormal step
MARGIN = 1e-4
# how far beside a kink the two-sided classes stand (tdf -+ y, |g| -+ tau), relative: the fp32 difference of two values 2 % apart keeps
# 6e-8 / 2e-2 = 3e-6 of itself, so a term made of nothing but such points still holds the suite's 1e-5
SIDE = 2e-2
W_EIK, W_HESS, W_HESS_ONLY = [1e4, 1e4, 0.0, 1e3], [1e4, 1e4, 1e4, 1e3], [1e4, 1e4, 1e4, 0.0]
W_SIREN, W_S2 = [3e3, 1e2, 1e2, 5e1], [1e5, 1e5]
COT_ONES, COT_MIXED = [1.0, 1.0, 1.0, 1.0], [0.5, 2.0, 3.0, 0.25]
SHAPES = [(1, 0), (1, 1), (5, 2), (64, 0), (65, 21), (257, 85), (700, 233)]
FILLER_H = np.diag([1.0, 2.0, 3.0])                        # the oracle's Hessian of a point that has none (off-surface: no term)


def f32(a):
    return np.asarray(a, dtype=F32)


def unit(rng):
    v = rng.standard_normal(3)
    return v / np.linalg.norm(v)


def rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    return q * np.sign(np.diag(r))


# ---- matrices of the eigensolver -----------------------------------------------------------------------------------------------------
def _rotated(rng, spectrum, scale=1.0):
    r = rotation(rng)
    h = (r * np.asarray(spectrum, dtype=np.float64)) @ r.T
    h = f32(0.5 * (h + h.T) * scale).astype(np.float64)
    return np.tril(h) + np.tril(h, -1).T


def eig_classes(seed=7, per=200):
    """name -> (k,3,3) float64 symmetric matrices with float32-representable entries: seeded random rotations of exact float32
    spectra, rounded to float32, and the structured ones written entry by entry."""
    rng = np.random.default_rng(seed)
    spec = lambda: np.sort(rng.integers(-32, 33, 3) / 8.0 + rng.integers(0, 2, 3) * np.array([0.0, 1 / 64, 1 / 32]))  # noqa: E731
    eps = float(np.finfo(F32).eps)
    out = {
        "generic": [_rotated(rng, spec()) for _ in range(per)],
        "double_top": [_rotated(rng, (-1.0, 2.0, 2.0)) for _ in range(per)],
        "double_bottom": [_rotated(rng, (1.0, 1.0, 3.0)) for _ in range(per)],
        "triple": [_rotated(rng, (s, s, s)) for s in (2.0, 0.0, -5.0) for _ in range(per // 3)]
                  + [np.eye(3) * s for s in (2.0, 0.0, -5.0)],
        "near_double_top": [_rotated(rng, (-1.0, 1.0, 1.0 + eps)) for _ in range(per // 2)],
        "near_double_bottom": [_rotated(rng, (1.0, 1.0 + eps, 3.0)) for _ in range(per // 2)],
        "spread_1e12": [_rotated(rng, (1e-6, 1.0, 1e6)) for _ in range(per)],
        "scaled_1e-30": [_rotated(rng, spec(), 1e-30) for _ in range(per)],
        "scaled_1e30": [_rotated(rng, spec(), 1e30) for _ in range(per)],
        "rank_one": [_rotated(rng, (0.0, 0.0, s)) for s in (3.0, -3.0) for _ in range(per // 2)],
    }
    diag = []
    for _ in range(per // 6):
        d = rng.permutation(np.arange(-8, 9))[:3] / 4.0
        diag += [np.diag(p) for p in itertools.permutations(d)]
    out["diagonal"] = [np.diag(p) for p in itertools.permutations((1.0, 2.0, 3.0))] + diag
    off = []
    for (i, j) in ((1, 0), (2, 0), (2, 1)):
        for e in (1e-20, -1e-20, 0.5, -2.0, 3.0):
            for d in (np.ones(3), np.zeros(3), np.array([1.0, 2.0, 3.0]), np.array([3.0, 1.0, 2.0])):
                h = np.diag(d)
                h[i, j] = h[j, i] = float(F32(e))
                off.append(h)
    out["one_offdiagonal"] = off
    return {k: np.stack(v) for k, v in out.items()}


def top_gap_rel(h):
    """(lam_2 - lam_1) / max|H| of the lower triangle in fp64 (0 for H = 0)"""
    lam = np.linalg.eigvalsh(h)
    scale = np.abs(np.tril(h)).max()
    return float((lam[2] - lam[1]) / scale) if scale > 0 else 0.0


# ---- Hessian-point classes of loss_s1 -------------------------------------------------------------------------------------------------
def _hess_classes(rng):
    """[(name, h (3,3) float32 as PLANTED, normal (3) float32, flags)], flags out of: cs0 (cos exactly 0), parallel (cos = +-1: Hbar at
    rounding level), upper (the upper triangle holds unrelated values)"""
    ec = eig_classes(seed=11, per=12)
    out = []

    def normal_for(h):
        lam, V = np.linalg.eigh(h)
        for _ in range(1000):
            m = f32(unit(rng) * rng.choice([1.0, 0.25, 7.0]))
            if 0.05 <= abs(m.astype(np.float64) @ V[:, 2]) / np.linalg.norm(m.astype(np.float64)) <= 0.95:
                return m
        raise AssertionError("no normal found")

    for name in ("generic", "double_bottom", "near_double_bottom", "spread_1e12", "scaled_1e-30", "scaled_1e30", "rank_one", "diagonal",
                 "one_offdiagonal"):
        good = [h for h in ec[name] if top_gap_rel(h) >= 1e-3]
        for h in good[:: max(1, len(good) // 3)][:3]:
            out.append((name, f32(h), normal_for(h), ()))
    out.append(("cs0_diag123", f32(np.diag([1.0, 2.0, 3.0])), f32([1.0, 0.0, 0.0]), ("cs0",)))
    for h, v in ((np.array([[2.0, 1, 0], [1, 2, 0], [0, 0, 0]]), [1.0, 1.0, 0.0]), (np.array([[1.0, 2, 2], [2, 1, 2], [2, 2, 1]]), [1.0, 1.0, 1.0])):
        out.append(("parallel+", f32(h), f32(v), ("parallel",)))
        out.append(("parallel-", f32(h), f32([-2.0 * c for c in v]), ("parallel",)))
    gen = [h for h in ec["generic"] if top_gap_rel(h) >= 1e-3]
    out.append(("zero_normal", f32(gen[-1]), f32([0.0, 0.0, 0.0]), ("cs0",)))
    h = np.array(gen[-2])
    hu = np.tril(h) + np.triu(rng.standard_normal((3, 3)) * 5.0, 1)
    out.append(("upper_unrelated", f32(hu), normal_for(h), ("upper",)))
    return out


def _g_of_norm(rng, norm):
    """a float32 vector of (close to) the given norm in a random direction; 0 stays exactly 0"""
    return f32(unit(rng) * norm)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
def _new_case(name, mode, n, n_hess, weights, alpha, cot, n_global):
    return {"name": name, "mode": mode, "n": n, "n_hess": n_hess, "weights": list(weights), "alpha": float(alpha), "cot": list(cot),
            "n_global": int(n_global if n_global is not None else n), "stats": None,
            "y": np.zeros(n, F32), "g": np.zeros((n, 3), F32), "h": np.zeros((n_hess, 3, 3), F32), "normals": np.zeros((n, 3), F32),
            "sdf": np.zeros(n, F32), "kind": [""] * n,
            # exact[k][p]: point p sits exactly on kink k and is left out of the margin; what it must give is asserted literally
            "exact": {k: np.zeros(n, bool) for k in ("y", "g", "cs", "gap")}, "exact_mu": False,
            "parallel": np.zeros(n, bool), "clamp": np.zeros(n, bool), "upper": np.zeros(n, bool),
            "nonfinite": [], "poison": [], "twin": None, "skip_terms": ()}


U_OFF = [FLT_MIN, 1e-6, 3e-3, None, 0.5, 3.0, -0.2]      # None: float32(1 / alpha)
Y_ON = [0.3, -0.3, 0.0, -0.0, DENORM]


def s1_case(name, n, n_hess, weights, alpha, cot, n_global=None, rot=0, extreme=False, plant=None):
    """loss_s1: the first n_hess points are the on-surface ones when the Hessian weight is on; without it every third point is."""
    rng = np.random.default_rng(1000 + rot)
    c = _new_case(name, "s1", n, n_hess, weights, alpha, cot, n_global)
    hess = weights[2] != 0
    hcls = _hess_classes(rng)
    y_on = Y_ON + ([1e30] if extreme else [])
    g_cls = ["zero", 1e-15, 1e-3, 1.0, 1e3, "tau+", "tau-"] + ([1e15] if extreme else [])
    off_cls = [(u, s) for u in U_OFF for s in (+1, -1)] + ["kink_y", "kink_yg"]
    for p in range(n):
        on = p < n_hess if hess else (p + rot) % 3 == 0
        i = p + rot
        kind = []
        if on:
            yv = y_on[i % len(y_on)]
            c["y"][p] = yv
            c["exact"]["y"][p] = (yv == 0)
            u = 0.0
            kind.append("on:y=%g" % yv if yv != 0 else ("on:y=-0" if np.signbit(F32(yv)) else "on:y=+0"))
        else:
            oc = off_cls[i % len(off_cls)]
            if isinstance(oc, str) and alpha != 100.0:
                oc = (0.5, +1)                              # tanh(5) != 1: no exact kink at alpha = 10
            if isinstance(oc, str):
                u = 0.5
                c["y"][p] = 0.5                             # tanhf(50) == 1: tdf == u == y, tau == 1
                c["exact"]["y"][p] = True
                kind.append(oc)
            else:
                u = float(F32(1.0 / alpha)) if oc[0] is None else float(F32(oc[0]))
                tdf = u * np.tanh(alpha * u)
                c["y"][p] = tdf + oc[1] * SIDE * max(abs(tdf), 1e-6)
                kind.append("off:u=%g%s" % (u, "+" if oc[1] > 0 else "-"))
        c["sdf"][p] = u
        tn = np.tanh(alpha * u)
        tau = abs(tn + u * alpha * (1.0 - tn * tn))
        gc = g_cls[i % len(g_cls)]
        if kind[0] == "kink_yg":
            c["g"][p] = [0.0, 0.0, -1.0]
            c["exact"]["g"][p] = True
            kind.append("g=(0,0,-1)")
        else:
            if isinstance(gc, str) and gc.startswith("tau"):
                norm = tau * (1.0 + (SIDE if gc == "tau+" else -SIDE))
                if not 1e-15 <= norm <= 1e15:
                    norm, gc = 1.0, "tau_fallback"
            else:
                norm = 0.0 if gc == "zero" else gc
                if norm > 0 and abs(norm - tau) < SIDE * max(norm, tau):   # the class's norm IS tau (1 at u = 0.5): step off the kink
                    norm, gc = tau * (1.0 + SIDE), "%g->tau+" % gc
            c["g"][p] = _g_of_norm(rng, norm)
            c["exact"]["g"][p] = (norm == 0.0 and tau == 0.0)      # |g| - tau == 0 - 0
            kind.append("g:%s" % gc)
        c["normals"][p] = f32(unit(rng))
        if p < n_hess:
            hname, h, m, flags = hcls[i % len(hcls)]
            c["h"][p], c["normals"][p] = h, m
            c["exact"]["cs"][p] = "cs0" in flags
            c["parallel"][p] = "parallel" in flags
            c["upper"][p] = "upper" in flags
            kind.append("h:" + hname)
        c["kind"][p] = " ".join(kind)
    if plant == "degenerate":                               # a degenerate top gap: Hbar is non-finite there and nowhere else
        twin = s1_case(name + "/twin", n, n_hess, weights, alpha, cot, n_global, rot, extreme)
        for p, h in zip(sorted({0, n_hess // 2, n_hess - 1}), itertools.cycle([np.diag([1.0, 2.0, 2.0]), np.zeros((3, 3))])):
            c["h"][p] = f32(h)
            c["normals"][p] = f32([0.48, 0.6, 0.64])
            c["exact"]["gap"][p] = True
            c["exact"]["cs"][p] = True                      # the top eigenvector is any vector of a plane: cos has no fixed value
            c["parallel"][p] = c["upper"][p] = False
            c["kind"][p] += " DEGENERATE"
            c["nonfinite"].append(p)
        c["twin"], c["skip_terms"] = twin, (2,)
    if plant == "poison":                                   # a Hessian-path point that is not on the surface
        twin = s1_case(name + "/twin", n, n_hess, weights, alpha, cot, n_global, rot, extreme)
        p = n_hess - 1
        c["sdf"][p] = 0.25
        c["kind"][p] += " POISON"
        c["poison"].append(p)
        c["twin"] = twin
    return c


def siren_case(name, n, weights, cot, n_global=None, rot=0):
    rng = np.random.default_rng(2000 + rot)
    c = _new_case(name, "siren", n, 0, weights, 100.0, cot, n_global)
    on_cls = ["generic", "zero_normal", "g=0", "gn=1e-9", "gn=1e-7", "g||+m", "g||-m"]
    off_cls = [0.0, 1e-4, -1e-4, 0.05, -0.05, 1.0, -1.0]
    for p in range(n):
        i = p + rot
        m = f32(unit(rng))
        g = f32(unit(rng) * rng.choice([0.5, 1.25, 2.0]))       # not 1: (|g| - 1)^2 of a rounded unit vector is 1e-15, which fp32 cannot hold
        if i % 2 == 0:
            oc = on_cls[(i // 2) % len(on_cls)]
            c["y"][p] = Y_ON[(i // 2) % len(Y_ON)]
            c["exact"]["y"][p] = c["y"][p] == 0
            if oc == "zero_normal":
                m = f32([0, 0, 0])
            elif oc == "g=0":
                g = f32([0, 0, 0])
            elif oc.startswith("gn="):
                g = _g_of_norm(rng, float(oc[3:]))
            elif oc.startswith("g||"):
                g = f32(m.astype(np.float64) * (0.75 if oc[3] == "+" else -1.5))
            c["clamp"][p] = oc in ("zero_normal", "g=0", "gn=1e-9")
            c["kind"][p] = "on:" + oc
        else:
            yv = off_cls[(i // 2) % len(off_cls)]
            c["y"][p] = yv
            c["sdf"][p] = [0.01, 0.3, -0.2][(i // 2) % 3]
            c["exact"]["y"][p] = (yv == 0)
            c["kind"][p] = "off:y=%g" % yv
        c["g"][p], c["normals"][p] = g, m
    return c


def s2_case(name, n, kind, rot=0):
    """loss_s2 on y alone.  kind: generic | none_on | one_on | identical | mu0 | stats_in"""
    rng = np.random.default_rng(3000 + rot)
    c = _new_case(name, "s2", n, 0, W_S2, 100.0, [1.0, 1.0, 0.0, 0.0] if rot % 2 == 0 else [0.5, 2.0, 0.0, 0.0], None)
    c["y"][:] = f32(rng.standard_normal(n) * 0.1 + 0.05)
    c["sdf"][:] = f32(np.where((np.arange(n) + rot) % 2 == 0, 0.0, 0.1 + 0.01 * rng.random(n)))
    c["g"][:] = f32(rng.standard_normal((n, 3)))
    c["normals"][:] = f32(rng.standard_normal((n, 3)))
    if kind == "none_on":
        c["sdf"][:] = 0.2
    elif kind == "one_on":
        c["sdf"][:] = 0.2
        c["sdf"][n // 2] = 0.0
    elif kind == "identical":
        c["sdf"][:] = 0.2
        on = np.linspace(0, n - 1, 8).astype(int)
        c["sdf"][on], c["y"][on] = 0.0, 0.25
    elif kind == "mu0":
        on = np.nonzero(c["sdf"] == 0)[0]
        on = on[: len(on) // 2 * 2]
        c["sdf"][:] = 0.2
        c["sdf"][on] = 0.0
        c["y"][on[1::2]] = -c["y"][on[0::2]]
        c["exact_mu"] = True
    elif kind == "stats_in":                                # the statistics of a larger global batch: not the local sums
        more = f32(rng.standard_normal(3 * n) * 0.1 + 0.07).astype(np.float64)
        yo = c["y"][c["sdf"] == 0].astype(np.float64)
        c["stats"] = np.array([yo.size + more.size, yo.sum() + more.sum(), (yo * yo).sum() + (more * more).sum()])
    if kind in ("none_on", "one_on", "identical"):
        c["nonfinite"] = [int(p) for p in np.nonzero(c["sdf"] == 0)[0]]
        c["exact_mu"] = kind == "none_on"
        twin = s2_case(name + "/twin", n, "generic", rot)
        twin["sdf"][:] = c["sdf"]                           # the same off-surface points; every on-surface point of the twin is generic
        c["twin"] = twin
    for p in range(n):
        c["kind"][p] = ("on" if c["sdf"][p] == 0 else "off") + ":" + kind
    return c


def all_cases():
    cs = []
    for k, (n, nh) in enumerate(SHAPES):
        alpha = 100.0 if k % 2 == 0 else 10.0
        cot = COT_ONES if k % 3 != 1 else COT_MIXED
        if nh == 0:
            cs.append(s1_case(f"s1 eik n={n}", n, 0, W_EIK, alpha, cot, rot=k))
            cs.append(s1_case(f"s1 eik n={n} alpha'", n, 0, W_EIK, 110.0 - alpha, COT_MIXED, rot=k + 7))
        else:
            cs.append(s1_case(f"s1 hess n={n},{nh}", n, nh, W_HESS, alpha, cot, rot=k))
            cs.append(s1_case(f"s1 hess-only n={n},{nh}", n, nh, W_HESS_ONLY, 110.0 - alpha, COT_MIXED, rot=k + 7))
    cs.append(s1_case("s1 hess n=257,85 n_global=3n", 257, 85, W_HESS, 100.0, COT_MIXED, n_global=771, rot=3))
    cs.append(s1_case("s1 hess weight, no on-surface point n=64", 64, 0, W_HESS, 100.0, COT_ONES, rot=5))
    cs.append(s1_case("s1 extreme n=65,21", 65, 21, W_HESS, 100.0, COT_ONES, rot=2, extreme=True))
    cs.append(s1_case("s1 extreme n=64", 64, 0, W_EIK, 10.0, COT_MIXED, rot=4, extreme=True))
    cs.append(s1_case("s1 degenerate n=65,21", 65, 21, W_HESS, 100.0, COT_MIXED, rot=1, plant="degenerate"))
    cs.append(s1_case("s1 degenerate n=700,233", 700, 233, W_HESS_ONLY, 10.0, COT_ONES, rot=6, plant="degenerate"))
    cs.append(s1_case("s1 poison n=65,21", 65, 21, W_HESS, 100.0, COT_ONES, rot=1, plant="poison"))
    for k, n in enumerate((1, 5, 64, 65, 257, 700)):
        cs.append(siren_case(f"siren n={n}", n, W_SIREN, COT_ONES if k % 2 else COT_MIXED, rot=k))
    cs.append(siren_case("siren n=257 n_global=3n", 257, W_SIREN, COT_ONES, n_global=771, rot=9))
    for k, n in enumerate((5, 64, 65, 257, 700)):
        cs.append(s2_case(f"s2 generic n={n}", n, "generic", rot=k))
    cs.append(s2_case("s2 no on-surface point n=65", 65, "none_on", rot=1))
    cs.append(s2_case("s2 one on-surface point n=1", 1, "one_on", rot=0))
    cs.append(s2_case("s2 one on-surface point n=257", 257, "one_on", rot=2))
    cs.append(s2_case("s2 identical on-surface points n=700", 700, "identical", rot=3))
    cs.append(s2_case("s2 mu=0 n=700", 700, "mu0", rot=4))
    cs.append(s2_case("s2 stats_in n=65", 65, "stats_in", rot=5))
    cs.append(s2_case("s2 stats_in n=700", 700, "stats_in", rot=6))
    return cs


# ---- the oracle's answer -----------------------------------------------------------------------------------------------------------
def oracle_inputs(c, symmetric_upper=False):
    """the case's float32 arrays as the fp64 oracle takes them: sdf (n,1), H (n,3,3) with FILLER_H where a point has no Hessian"""
    n, nh = c["n"], c["n_hess"]
    H = np.tile(FILLER_H, (n, 1, 1))
    H[:nh] = c["h"].astype(np.float64)
    return (c["y"].astype(np.float64), c["g"].astype(np.float64), H, c["normals"].astype(np.float64),
            c["sdf"].astype(np.float64).reshape(n, 1))


def reference(c):
    """The oracle in fp64 on the case's float32 inputs, with N = n_global and the upstream cotangents applied: terms (4), stats (3) or
    None, ybar (n), gbar (n,3), hbar (n_hess,3,3), and what the margin needs (lam, cos).  The oracle divides by the local n and returns
    the cotangents of the plain SUM of its terms; both are linear, so N = n_global is the factor n / n_global and the cotangent of
    sum_i cot_i term_i is the cotangent of the sum at weights w_i cot_i."""
    y, g, H, m, sdf = oracle_inputs(c)
    n, nh, w = c["n"], c["n_hess"], np.asarray(c["weights"], dtype=np.float64)
    wc = w * np.asarray(c["cot"], dtype=np.float64)[: len(w)]
    scale = n / c["n_global"]
    out = {"stats": None, "hbar": np.zeros((nh, 3, 3)), "lam": None, "cos": None}
    with np.errstate(all="ignore"):
        if c["mode"] == "s1":
            terms, cot = O.loss_s1_terms(y, g, H, m, sdf, list(w), c["alpha"])
            _, cotc = O.loss_s1_terms(y, g, H, m, sdf, list(wc), c["alpha"])
            if w[2] != 0:
                out["hbar"], out["lam"], out["cos"] = cotc["Hbar"][:nh] * scale, cot["lam"], cot["cos"]
        elif c["mode"] == "siren":
            terms, cot = O.loss_siren_terms(y, g, m, sdf, list(w))
            _, cotc = O.loss_siren_terms(y, g, m, sdf, list(wc))
        else:
            terms, _ = O.loss_s2_terms(y, sdf, list(w))
            _, cotc = O.loss_s2_terms(y, sdf, list(wc), stats=None if c["stats"] is None else tuple(c["stats"]))
            yo = y[sdf[:, 0] == 0]
            out["stats"] = np.array([yo.size, yo.sum(), (yo * yo).sum()])
            scale = 1.0                                     # loss_s2 has no 1 / N: its statistics carry the count
        t = np.array([float(v) for v in terms.values()] + [0.0] * (4 - len(terms))) * scale
    out["terms"] = t
    out["ybar"] = cotc["ybar"] * scale
    out["gbar"] = np.zeros((n, 3)) if cotc.get("gbar") is None else cotc["gbar"] * scale
    return out


def margin(c, ref=None):
    """(smallest relative distance of a non-exact point to a kink, which kink, which point) under the oracle's fp64 evaluation: tdf - y
    and |g| - tau relative to the larger of the two, cos as it is, lam_2 - lam_j relative to max|H|, mu relative to the largest |y| on
    the surface; loss_siren: y, and |g| against the 1e-8 clamp of the cosine."""
    ref = ref or reference(c)
    y, g, H, m, sdf = oracle_inputs(c)
    u = sdf[:, 0]
    on = u == 0
    worst = (np.inf, "", -1)

    def take(dist, kink, skip):
        nonlocal worst
        d = np.where(skip, np.inf, dist)
        if d.size and d.min() < worst[0]:
            worst = (float(d.min()), kink, int(d.argmin()))

    rel = lambda a, b: np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300)  # noqa: E731
    gn = np.sqrt((g * g).sum(-1))
    if c["mode"] == "s1":
        tn = np.tanh(c["alpha"] * u)
        take(rel(np.where(on, 0.0, u * tn), y), "tdf-y", c["exact"]["y"])
        if c["weights"][3] != 0:
            take(rel(gn, np.abs(tn + u * c["alpha"] * (1 - tn * tn))), "gn-tau", c["exact"]["g"])
        if c["weights"][2] != 0 and c["n_hess"]:
            nh = c["n_hess"]
            take(np.abs(ref["cos"][:nh]), "cs", c["exact"]["cs"][:nh])
            hs = np.abs(np.tril(H[:nh])).max((1, 2))
            for j in (0, 1):
                take((ref["lam"][:nh, 2] - ref["lam"][:nh, j]) / np.maximum(hs, 1e-300), "lam2-lam%d" % j, c["exact"]["gap"][:nh])
    elif c["mode"] == "siren":
        take(np.where(y != 0, 1.0, 0.0), "y", c["exact"]["y"])
        take(rel(gn, 1e-8), "gn-clamp", ~on)
    else:
        yo = y[on]
        if not c["exact_mu"] and yo.size:
            take(np.array([abs(yo.mean()) / np.abs(yo).max()]), "mu", np.zeros(1, bool))
    return worst
