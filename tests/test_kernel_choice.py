# coding: utf-8
"""CPU: which kernel a launch gets is decided in one place (csrc/dudf_variants.h; dudf_debug_kernel_choice asks it without
launching anything).

  * coverage — the stash mask a workspace is promised (dudf_stash_mode) has a kernel for every sweep of a training step and for
    the weight-gradient GEMM, and that kernel is built for exactly this mask: over every width, depths on both sides of the 32-
    and 64-layer limits, batches on both sides of the 32-bit-offset limit and every combination of the options that select kernels;
  * reachability — every name the chooser returns is a kernel of the built library, and every sweep / GEMM kernel of the library
    is chosen by some request (or listed below with the reason);
  * the instantiation tables hold what the ISA contract test pins."""
import ctypes
import itertools
import re

from diffudf_amd import _lib
from isa_contract import variant_table

WIDTHS, DEPTHS, SIZES = (32, 64, 128, 256, 512), (1, 2, 8, 32, 33, 64, 65), (1, 29970, 5_000_000)
OPTIONS = (("stash", (7, 6, 0)), ("pair_launch", (1, 0)), ("split_quads", (1, 0)), ("split", (1, 0)), ("sweep_family", (1, 0)),
           ("wgrad_family", (0, 1, 2)), ("wgrad_tr", (0, 1)), ("wgrad_buffers", (4, 3)), ("deterministic", (0, 1)))
PAIR, WGRAD, QUERY = 16, -1, 16
S, C, TRAIN, HAVE_E = 1, 2, 4, 8
ALL = S | C | TRAIN | HAVE_E
# a training step's sweeps: (sweep, flags); loss_s2 runs the adjoint reverse sweep without df/dx terms
STEP = ((0, ALL), (1, ALL), (2, TRAIN | HAVE_E), (3, TRAIN | HAVE_E), (3, TRAIN))
# query launches (flags | QUERY): value, value + gradient / Hessian, jets
QUERIES = ((0, HAVE_E), (0, C | HAVE_E), (1, HAVE_E), (8, HAVE_E))
# kernels of dudf_sweep.hip / dudf_sweep_bf16.hip / dudf_sweep_wide.hip / dudf_wgrad.hip that no request of the enumeration reaches — reported, not removed
UNREACHED = {}          # name: reason (none at present)
# ... and the kernels of those files that are not subject to a choice (packing, thin layers): one per width
FIXED = ("pack_bf16_kernel", "pack_f16_kernel", "prep_kernel", "wgrad_small_kernel", "wgrad_small_p24_kernel")


def mask_of(name):
    """the stash mask a kernel is built for, from its name"""
    if name.startswith("sweep_pair_kernel"):
        return int(name[:-1].split(",")[-1])
    if name.startswith(("sweep_f16p_", "wgrad_hidden_f16p24_")):
        return 7
    return 6 if name.startswith(("sweep_f16r_", "sweep_w16r_")) else 0


def library_kernels():
    """kernel symbols of the built library's device code (every kernel has a descriptor symbol <mangled name>.kd)"""
    out = set()
    for sym in set(re.findall(rb"_ZN12_GLOBAL__N_1(\w+?)\.kd", open(_lib.LIB_PATH, "rb").read())):
        sym = sym.decode()
        n = int(re.match(r"\d+", sym).group(0))
        name, rest = sym[len(str(n)):][:n], sym[len(str(n)) + n:]
        args = re.match(r"I((?:Li\d+E)+)E", rest)
        out.add(name + ("<%s>" % ",".join(re.findall(r"Li(\d+)E", args.group(1))) if args else ""))
    return out


def test_every_promised_stash_mask_has_its_kernels_and_every_kernel_is_reachable():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(128)
    chosen, findings = set(), []

    def choice(cfg, n, nh, which, flags):
        rc = lib.dudf_debug_kernel_choice(ctypes.byref(cfg), n, nh, which, flags, buf, len(buf))
        if rc == 0:
            chosen.add(buf.value.decode())
        return rc, buf.value.decode()

    try:
        for values in itertools.product(*(v for _, v in OPTIONS)):
            opts = dict(zip((k for k, _ in OPTIONS), values))
            for k, v in opts.items():
                assert lib.dudf_set_option(k.encode(), v) == 0
            for H, L, n in itertools.product(WIDTHS, DEPTHS, SIZES):
                cfg = _lib.NetCfg(3, L, H, 30.0)
                for nh in (0, max(1, n // 3)):
                    mask = lib.dudf_stash_mode(ctypes.byref(cfg), n, nh)
                    where = (H, L, n, nh, tuple(values), mask)
                    assert mask in (0, 6, 7), where
                    for base, flags in STEP:
                        ranges = ([base + 4] if nh else []) + ([base] if n > nh else [])
                        if len(ranges) == 2:                       # one grid for both, or one launch after the other
                            rc, name = choice(cfg, n, nh, base | PAIR, flags)
                            if rc == 0:
                                if mask_of(name) != mask:
                                    findings.append(where + (name,))
                                continue
                        for which in ranges:
                            rc, name = choice(cfg, n, nh, which, flags)
                            if rc != 0 or mask_of(name) != mask:
                                findings.append(where + (which, flags, rc, name))
                    if L >= 2:
                        rc, name = choice(cfg, n, nh, WGRAD, 0)
                        if rc != 0 or (mask_of(name) & 1) != (mask & 1):
                            findings.append(where + ("wgrad", rc, name))
                if n == 1:                                         # the query kernels do not depend on the batch
                    for which, flags in QUERIES:
                        for w, k in ((which, 0), (which + 4 if which < 4 else which, n)):
                            rc, name = choice(cfg, n, k, w, flags | QUERY)
                            assert rc == 0, (H, L, w, flags, opts, rc)
    finally:
        lib.dudf_reset_options()
    assert not findings, (len(findings), findings[:10])
    built = library_kernels()
    assert chosen <= built, sorted(chosen - built)
    ours = {k for k in built if k.startswith(("sweep_", "wgrad_hidden_"))}
    assert len(ours) == 60 + 129 + 13                   # dudf_sweep.hip, dudf_sweep_bf16.hip + dudf_sweep_wide.hip (138 with the 9 packing kernels of dudf_prep.hip), dudf_wgrad.hip
    assert {k.split("<")[0] for k in built - ours if k.split("<")[0] in FIXED} == set(FIXED)
    assert ours - chosen == set(UNREACHED), sorted((ours - chosen) ^ set(UNREACHED))


def test_instantiation_tables_are_what_the_isa_contract_pins():
    """tests/test_isa_contract.py takes its key sets from the table; their contents are pinned here."""
    sweep = variant_table("kSweepVariants")
    assert {(s, f) for s, f, _ in sweep} == {(0, 3), (0, 2), (0, 0), (1, 1), (1, 0), (2, 0), (3, 1), (3, 0),
                                             (4, 1), (4, 0), (5, 1), (5, 0), (6, 0), (7, 0), (8, 0)}
    assert {(s, f) for s, f, p in sweep if p} == {(0, 3), (1, 1), (2, 0), (3, 1), (3, 0), (4, 1), (5, 1), (6, 0), (7, 0)}
    assert len(sweep) == 15 and len(variant_table("kWideVariants")) == 13 and len(variant_table("kF32Variants")) == 12
    # 138 kernels of dudf_sweep_bf16.hip, dudf_sweep_wide.hip and dudf_prep.hip: two widths x two families x 15, 2 x 9 for the 24-bit stash, 2 x 13 + 9 at 512, 16 pair
    # kernels (4 sweeps x {bf16x6 quads, fp16x3 quads, masks 6 and 7}), and the 3 x 3 packing kernels
    assert 2 * 2 * 15 + 2 * 9 + 2 * 13 + 9 + 4 * len(variant_table("kPairVariants")) + 9 == 138


def test_design_table_rows_are_the_choosers_answers():
    """DESIGN.md §3.1 "Who runs which build": the rows that name one kernel (8 layers, 29 970 points) are what the chooser says."""
    import os
    lib = _lib.load()
    buf = ctypes.create_string_buffer(128)
    doc = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "DESIGN.md")).read()
    rows = [(256, {}, 0, ALL, "sweep_f16p_np_kernel<256,0,3>", "7 (default)"), (256, {"stash": 6}, 0, ALL, "sweep_f16r_np_kernel<256,0,3>", "6"),
            (256, {"stash": 0}, 0, ALL, "sweep_f16_np_kernel<256,0,3>", "0"), (256, {}, 0, HAVE_E | QUERY, "sweep_f16_np_kernel<256,0,0>", "0"),
            (256, {"split": 0}, 0, ALL, "sweep_bf16_np_kernel<256,0,3>", "0"), (128, {}, 0, ALL, "sweep_f16_np_kernel<128,0,3>", "0"),
            (128, {"split": 0}, 0, ALL, "sweep_bf16_np_kernel<128,0,3>", "0"), (512, {}, 0, ALL, "sweep_w16r_kernel<0,3>", "6 (default)"),
            (512, {"stash": 0}, 0, ALL, "sweep_w16_kernel<0,3>", "0"), (512, {}, 0, HAVE_E | QUERY, "sweep_w16_kernel<0,1>", "0"),
            (512, {"split": 0}, 0, ALL, "sweep_w_kernel<0,3>", "0"), (256, {}, WGRAD, 0, "wgrad_hidden_f16p24_kernel<256,25>", "7"),
            (256, {"wgrad_buffers": 3}, WGRAD, 0, "wgrad_hidden_f16p24_kernel<256,9>", "7"), (512, {}, WGRAD, 0, "wgrad_hidden_f16p_kernel<256,9>", "0, 6"),
            (256, {"split": 0}, WGRAD, 0, "wgrad_hidden_bf16p_kernel<256,9>", "0")]
    try:
        for H, opts, which, flags, kernel, mask in rows:
            lib.dudf_reset_options()
            for k, v in opts.items():
                assert lib.dudf_set_option(k.encode(), v) == 0
            cfg = _lib.NetCfg(3, 8, H, 30.0)
            assert lib.dudf_debug_kernel_choice(ctypes.byref(cfg), 29970, 0, which, flags, buf, len(buf)) == 0
            assert buf.value.decode() == kernel, (H, opts, which, buf.value, kernel)
            line = [ln for ln in doc.split("\n") if ln.startswith("|") and "`%s`" % kernel in ln]
            assert len(line) == 1 and ("| %s |" % mask) in line[0] and str(H) in line[0].split("|")[1], (kernel, line)
    finally:
        lib.dudf_reset_options()
