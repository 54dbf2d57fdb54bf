# coding: utf-8
"""CPU (needs hipcc, no GPU): the hand-counted `s_waitcnt vmcnt(N)` behind the inline-asm LDS-DMA of the H=256
sweep kernels must never be larger than the number of vector-memory instructions hipcc actually placed between
the last DMA piece and the wait — otherwise a weight chunk could be read before it has landed."""
import os
import shutil
import pytest

import sys, os as _os
sys.path.insert(0, _os.path.dirname(_os.path.abspath(__file__)))
from isa_contract import analyse, analyse_bf16, analyse_f16, analyse_wgrad_presplit, emit_asm, variant_table

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16_SRC = os.path.join(REPO, "diffudf_amd", "csrc", "dudf_sweep_bf16.hip")
# the built (SW, FL) variants of the 256-wide bf16x6 / fp16x3 kernels, and those with builds for a 24-bit stash: the instantiation
# table the launchers dispatch through (tests/test_kernel_choice.py pins its contents)
SWEEP_KEYS = {(sw, fl) for sw, fl, p24 in variant_table("kSweepVariants")}
P24_KEYS = {(sw, fl) for sw, fl, p24 in variant_table("kSweepVariants") if p24}


@pytest.fixture(scope="module")
def bf16_asm(tmp_path_factory):
    """Assembly of dudf_sweep_bf16.hip (the 128- and 256-wide kernels: the unit holds what the analysers below read, the 512-wide
    kernels and the packing kernels are units of their own) per flag set, emitted once per test session (three builds, in parallel)."""
    from concurrent.futures import ThreadPoolExecutor
    d = tmp_path_factory.mktemp("sweep_bf16_asm")
    builds = {"late0": ("-DDUDF_LATE_FORCE=0",), "late1": ("-DDUDF_LATE_FORCE=1",), "ship": ()}
    paths = {k: str(d / f"{k}.s") for k in builds}
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("needs hipcc")
    with ThreadPoolExecutor(3) as ex:
        list(ex.map(lambda k: emit_asm(BF16_SRC, paths[k], flags=builds[k]), builds))
    return paths


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_dma_wait_counts(tmp_path):
    asm = str(tmp_path / "sweep.s")
    emit_asm(os.path.join(REPO, "diffudf_amd", "csrc", "dudf_sweep.hip"), asm)
    res = analyse(asm)
    assert len(res) >= 7
    for key, v in res.items():
        assert v["pairs"], key
        for counted, n in v["pairs"]:
            assert counted >= n, f"sweep_kernel<256,{key[0]},{key[1]}>: vmcnt({n}) but only {counted} younger ops"
    # the training variants must not spill
    for key in ((0, 3), (1, 1), (2, 0), (3, 1), (3, 0)):
        assert res[key]["scratch"] == 0, key


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_bf16_sweep_wait_counts(tmp_path, bf16_asm):
    """dudf_sweep_bf16.hip: every step's counted wait leaves exactly this step's DMA pieces and two steps of stash
    traffic in flight (a larger N would let a wave read a weight chunk that has not landed; a smaller one only
    stalls), the idle-wave loop waits for all but its newest pieces, and nothing spills at 2 waves per SIMD."""
    src = os.path.join(REPO, "diffudf_amd", "csrc", "dudf_sweep_bf16.hip")
    keys = SWEEP_KEYS                                                                      # + the Hessian-quad variants
    # The shipped kernels hold BOTH halves' program orders behind a wave-uniform branch (waves 0-3: DMA pieces and
    # operand loads at the top of a step, tail early; waves 4-7: MFMAs first, then DMA pieces, loads and tail).  The
    # count is a property of each order: check each one in a build where that order is the only one (straight-line steps).
    for force in (0, 1):
        asm = bf16_asm[f"late{force}"]
        res = analyse_bf16(asm, ndma=12)
        assert set(res) == keys
        for key, v in res.items():
            assert v["scratch"] == 0, (force, key)
            if force == 1:
                continue        # the late order belongs to waves 4-7, which issue no DMA pieces and do not wait for any
                                # (every variant: `dma2` and the hand-written wait sit behind `wave < NWB / 2`)
            for dma, ops, n in v["steps"]:
                assert n <= 2 * ops + dma, f"late={force} sweep_bf16_kernel<256,{key[0]},{key[1]}>: vmcnt({n}) with {ops} ops/step"
            # the unrolled steps of a layer (the first entry also carries the first layer's prologue traffic): waves 0-3 issue
            # the 6 pieces of their SIMD partner as well -> 12 per step
            kmin = min(s[1] for s in v["steps"] if s[0] == 12)
            steady = [s for s in v["steps"] if s[0] == 12 and s[1] == kmin]
            assert len(steady) >= 7, (force, key, v["steps"])
            for dma, ops, n in steady:
                assert n == 2 * ops + dma, (force, key, dma, ops, n)   # and not needlessly small either
            assert any(s == (12, 0, 12) or s[2] == 12 for s in v["steps"]) or v["idle"], key   # the idle-wave loop's vmcnt(2 NDMA)
    # the shipped build: same kernels, nothing spills at 2 waves per SIMD, and the forward sweeps are the builds
    # without packed fp32 instructions (they do not execute beside the SIMD partner's MFMAs)
    asm = bf16_asm["ship"]
    res = analyse_bf16(asm, ndma=12)
    assert set(res) == keys
    assert all(v["scratch"] == 0 for v in res.values())
    txt = open(asm).read()
    import re
    for m in re.finditer(r"^_ZN\w*sweep_bf16_np_kernelILi256ELi0ELi\dE\w*:", txt, re.M):
        body = txt[m.end():txt.index("s_endpgm", m.end())]
        assert "v_pk_fma_f32" not in body and "v_pk_mul_f32" not in body and "v_pk_add_f32" not in body
    assert len(re.findall(r"^_ZN\w*sweep_bf16_np_kernelILi256ELi0ELi\dE\w*:", txt, re.M)) == 3


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_f16_sweep_wait_counts(tmp_path, bf16_asm):
    """fp16x3 sweep kernels: replay of the vector-memory FIFO (tests/isa_contract.py::analyse_f16) for each half's program
    order — no hand-written wait may leave a DMA piece of the chunk the next step reads in flight, the steady-state waits
    are as loose as that allows, nothing spills, and the kernels are the builds without packed fp32 instructions."""
    import re
    src = os.path.join(REPO, "diffudf_amd", "csrc", "dudf_sweep_bf16.hip")
    for force in (0, 1):
        asm = bf16_asm[f"late{force}"]
        res = analyse_f16(asm)
        assert set(res) == SWEEP_KEYS, sorted(res)   # + the Hessian quads' training / query sweeps, the jets
        for key, v in res.items():
            assert len(v["waits"]) >= 8, (force, key, v["waits"])
            for n, late, slack in v["waits"]:
                assert late == 0, f"late={force} sweep_f16_kernel<256,{key[0]},{key[1]}>: vmcnt({n}) leaves {late} pieces of the next chunk in flight"
            # the forward sweep has no operand loads: its hand-written wait is the only one of a step and must not be needlessly
            # strict (the other sweeps' operand waits, placed by the compiler, retire the older DMA pieces anyway)
            if key[0] == 0 and force == 0:
                assert sum(1 for n, late, slack in v["waits"] if slack == 0) >= 7, (force, key, v["waits"])
    # the builds that keep stash arrays at 24 bits (training variants of the plain columns and of the quads) — f16r: R, E and C (stash
    # mask 6), f16p: S, Q, A, Z as well (mask 7, the default of 256-wide networks): same step structure, dwordx3 stash accesses — the
    # same replay must hold
    p24_keys = P24_KEYS
    for fam in ("f16r", "f16p"):
        for force in (0, 1):
            res = analyse_f16(bf16_asm[f"late{force}"], family=fam)
            assert set(res) == p24_keys, (fam, sorted(res))
            for key, v in res.items():
                assert len(v["waits"]) >= 8, (fam, force, key, v["waits"])
                for n, late, slack in v["waits"]:
                    assert late == 0, f"late={force} sweep_{fam}_kernel<256,{key[0]},{key[1]}>: vmcnt({n}) leaves {late} pieces of the next chunk in flight"
    # Nothing spills inside a k-block step — with ONE exception in both 24-bit families: the adjoint forward sweep (two 24-bit
    # arrays: it unpacks R and packs E) sits at 256 registers and parks one value inside a step.  An extra vector-memory
    # operation there only makes the counted waits stricter (a cost, not a hazard); measured, the sweep is still 10 % faster than
    # its fp32-stash build (profiles/r04_p24_ab2.txt).
    for fam in ("f16r", "f16p"):
        ship = analyse_f16(bf16_asm["ship"], family=fam)
        assert len(ship) == 9, (fam, sorted(ship))
        for key, v in ship.items():
            assert v["scratch_hot"] <= (1 if key == (2, 0) else 0) and v["scratch"] <= 32, (fam, key, v["scratch"], v["scratch_hot"])   # (cold: prologue / end-of-pass flush of the side values)
            assert v["scratch_pass"] <= 4, (fam, key, v["scratch_pass"])     # (once per pass, in the f32 output stage: the fixed-point reverse sweep reloads 3)
    ship = analyse_f16(bf16_asm["ship"])                # the shipped kernels (both orders behind a wave-uniform branch): nothing spills inside a loop (a few dwords of cold address spills in the prologue are tolerated)
    # (the adjoint forward sweep parks ~20 dwords around its pass: prologue addresses, the end-of-pass flush of the staged ebound)
    assert len(ship) == 15 and all(v["scratch_hot"] == 0 and v["scratch"] <= (24 if k == (2, 0) else 8) for k, v in ship.items()), \
        {k: (v["scratch"], v["scratch_hot"]) for k, v in ship.items()}
    txt = open(bf16_asm["ship"]).read()
    names = re.findall(r"^(_ZN\w*sweep_f16_np_kernelILi256ELi\dELi\dE\w*):", txt, re.M)
    assert len(names) >= 3
    for m in re.finditer(r"^_ZN\w*sweep_f16_np_kernelILi256ELi\dELi\dE\w*:", txt, re.M):
        body = txt[m.end():txt.index("s_endpgm", m.end())]
        assert "v_pk_fma_f32" not in body and "v_pk_mul_f32" not in body and "v_pk_add_f32" not in body
        assert body.count("v_fma_mix_f32") >= 64            # the residual of the fp16 split reads the fp16 half directly


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_wgrad_register_staging_contract(tmp_path):
    """dudf_wgrad.hip, cooperative-split kernel: three stages (12 loads) travel in registers across the loop's back edge
    behind hand-counted waits; no instruction may read or write such a register before its wait."""
    asm = str(tmp_path / "wgrad.s")
    emit_asm(os.path.join(REPO, "diffudf_amd", "csrc", "dudf_wgrad.hip"), asm)
    # VAR 9 = the cooperative-split body with three image buffers (25, below: four)
    res = analyse_wgrad_presplit(asm, 9)
    assert res["loads"] == 12 and res["carried"] == 12, res
    assert not res["bad"], res["bad"][:5]
    assert res["scratch"] == 0
    # the fp16x3 build of the same body (round 3: the default): same contract
    res = analyse_wgrad_presplit(asm, 9, "f16")
    assert res["loads"] == 12 and res["carried"] == 12 and not res["bad"] and res["scratch"] == 0, res
    # ... and of the build that reads 24-bit tile-major fixed-point operands (dwordx3 staging loads + one dword of column scale per
    # register set, transposed LDS fragment reads): 5 loads per set
    for var in (25, 9):                                   # 25 = the default (four image buffers), 9 = option wgrad_buffers = 3
        res = analyse_wgrad_presplit(asm, var, "f16p24")
        assert res["loads"] == 15 and res["carried"] == 15 and not res["bad"] and res["scratch"] == 0, (var, res)
    # ... and of the build that stages the fp32 rows through the same [column][feature] image (option wgrad_tr): 4 loads per set
    res = analyse_wgrad_presplit(asm, 9, "f16tr")
    assert res["loads"] == 12 and res["carried"] == 12 and not res["bad"] and res["scratch"] == 0, res
    txt = open(asm).read()
    import re
    m = re.search(r"^(_ZN\w*wgrad_hidden_f16p24_kernelILi256ELi25E\w*):", txt, re.M)
    body = txt[m.end():re.compile(r"^\.Lfunc_end\d+:", re.M).search(txt, m.end()).start()]
    assert body.count("ds_read_b64_tr_b16") >= 24 and "global_load_dwordx4" not in body

