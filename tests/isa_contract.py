# coding: utf-8
"""Static check of the built sweep kernels' instruction streams (helper for tests/test_isa_contract.py).

The H=256 sweep kernels stage weights with inline-asm LDS-DMA that hipcc does not count, and wait for it with
hand-written counted `s_waitcnt vmcnt(N)`.  N must equal the number of compiler-issued vector-memory
instructions between the last DMA piece and that wait.  This parses the assembly hipcc emits for
dudf_sweep.hip and returns, per kernel, the list of (counted, N) pairs.
"""
import re
import subprocess
import sys


def emit_asm(src, out, flags=()):
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S",
                    "--cuda-device-only", *flags, src, "-o", out], check=True, stderr=subprocess.DEVNULL)


def variant_table(name):
    """The built (SW, FL, p24) variants of a kernel family: the instantiation table `name` of csrc/dudf_variants.h."""
    import os
    hdr = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "diffudf_amd", "csrc", "dudf_variants.h")
    m = re.search(r"constexpr\s+DudfVariant\s+%s\s*\[\s*\]\s*=\s*\{(.*?)\}\s*;" % name, open(hdr).read(), re.S)
    rows = re.findall(r"\{\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*\}", m.group(1)) if m else []
    assert rows, "no table `%s` of {sw, fl, p24} rows in %s" % (name, hdr)
    return [tuple(int(v) for v in r) for r in rows]


def analyse(asm_path):
    txt = open(asm_path).read()
    out = {}
    for m in re.finditer(r"^(_ZN\w*(?:sweep_kernelILi256ELi(\d)ELi(\d)E|step_kernelILi256ELi(\d)E)\w*):[^\n]*$", txt, re.M):
        end = txt.index("s_endpgm", m.end())
        body = txt[m.end():end]
        pairs, drains, cnt, scratch, in_asm = [], [], None, 0, False
        for ln in body.split("\n"):
            t = ln.strip()
            if t.startswith(";;#ASMSTART"):
                in_asm = True
            elif t.startswith(";;#ASMEND"):
                in_asm = False
            if t.startswith("scratch_"):
                scratch += 1
            if t.startswith("global_load_lds"):
                cnt = 0
            elif re.match(r"(global_load|global_store|global_atomic|buffer_|scratch_|flat_)", t):
                if cnt is not None:
                    cnt += 1
            elif t.startswith("s_waitcnt") and "vmcnt" in t and cnt is not None:
                n = int(re.search(r"vmcnt\((\d+)\)", t).group(1))
                if in_asm:                       # the hand-written dma_wait
                    pairs.append((cnt, n))
                    cnt = None
                else:                            # compiler wait while a DMA is in flight: legal, may drain it early
                    drains.append((cnt, n))
        key = (int(m.group(2)), int(m.group(3))) if m.group(2) is not None else ("step", int(m.group(4)))
        out[key] = {"pairs": pairs, "drains": drains, "scratch": scratch}
    return out


if __name__ == "__main__":
    for k, v in sorted(analyse(sys.argv[1]).items(), key=str):
        print(k, v["scratch"], v["pairs"], "drains:", v["drains"])


def analyse_bf16(asm_path, ndma=6):
    """bf16x6 sweep kernels (dudf_sweep_bf16.hip): weight chunks are fetched TWO steps ahead, so the hand-written wait
    at the end of a step must leave in flight this step's DMA pieces plus two steps' compiler-issued stash traffic:
    N == 2 * (vector-memory instructions hipcc placed in the step) + ndma.  Returns per kernel
    {"steps": [(dma pieces, compiler ops, N)], "idle": [N of the idle-wave loop], "scratch": count}."""
    txt = open(asm_path).read()
    out = {}
    for m in re.finditer(r"^(_ZN\w*sweep_bf16_(?:np_)?kernelILi256ELi(\d)ELi(\d)E\w*):[^\n]*$", txt, re.M):
        end = txt.index("s_endpgm", m.end())
        body = txt[m.end():end]
        in_asm, dma, other, scratch, steps, idle = False, 0, 0, 0, [], []
        for ln in body.split("\n"):
            t = ln.strip()
            if t.startswith(";;#ASMSTART"):
                in_asm = True
            elif t.startswith(";;#ASMEND"):
                in_asm = False
            if t.startswith("scratch_"):
                scratch += 1
            if t.startswith("global_load_lds"):
                dma += 1
            elif re.match(r"(global_load|global_store|global_atomic|buffer_|flat_)", t):
                other += 1
            elif t.startswith("s_waitcnt") and "vmcnt" in t and in_asm:
                n = int(re.search(r"vmcnt\((\d+)\)", t).group(1))
                if n == 0:
                    continue                     # drains (tile start, last two steps): always safe
                if n == ndma and other == 0:
                    idle.append(n)
                else:
                    steps.append((dma, other, n))
                dma = other = 0
        out[(int(m.group(2)), int(m.group(3)))] = {"steps": steps, "idle": idle, "scratch": scratch}
    return out


def _vregs(tok):
    out = set()
    for a, b in re.findall(r"v\[(\d+):(\d+)\]", tok):
        out |= set(range(int(a), int(b) + 1))
    for a in re.findall(r"(?<![\[\w])v(\d+)(?![\d:\]])", tok):
        out.add(int(a))
    return out


def analyse_wgrad_presplit(asm_path, var=0, kernel="p"):
    """wgrad_hidden_bf16p_kernel<256> stages the stash through REGISTERS with inline-asm loads and hand-counted vmcnt
    waits inside its steady-state loop (hipcc does not know those registers are in flight).  Finds that loop (the
    self-looping basic block that holds the MFMAs and the asm loads), replays it twice with a FIFO of the loads — the
    second pass starts with what the first left in flight — and returns the instructions that touch a destination
    register of a load still in flight (must be none), the loads per pass and the loads in flight across the back edge."""
    txt = open(asm_path).read()
    if kernel == "f16":        # the fp16x3 build of the same body
        m = re.search(r"^(_ZN\w*wgrad_hidden_f16p_kernelILi256ELi%dE\w*):" % var, txt, re.M)
    elif kernel == "f16p24":   # ... reading 24-bit tile-major operands: dwordx3 staging loads
        m = re.search(r"^(_ZN\w*wgrad_hidden_f16p24_kernelILi256ELi%dE\w*):" % var, txt, re.M)
    elif kernel == "f16tr":    # ... reading the fp32 rows through the [column][feature] image: dwordx4 staging loads, transposed fragment reads
        m = re.search(r"^(_ZN\w*wgrad_hidden_f16tr_kernelILi256ELi%dE\w*):" % var, txt, re.M)
    elif kernel == "q":        # the fragment-prefetching kernel: two register sets (8 loads) per pass of its two-stage loop
        m = re.search(r"^(_ZN\w*wgrad_hidden_bf16q_kernelILi256E\w*):", txt, re.M)
    else:
        m = re.search(r"^(_ZN\w*wgrad_hidden_bf16p_kernelILi256ELi%dE\w*):" % var, txt, re.M)
    # (to the end of the FUNCTION, not to the first s_endpgm: the kernel returns early for the padding blocks of its 1-D grid)
    body = txt[m.end():re.compile(r"^\.Lfunc_end\d+:", re.M).search(txt, m.end()).start()].split("\n")
    blocks, cur, name = [], [], "entry"
    for ln in body:
        t = ln.strip()
        if re.match(r"^\.LBB\d+_\d+:", t):
            blocks.append((name, cur))
            name, cur = t.split(":")[0], []
        else:
            cur.append(t)
    blocks.append((name, cur))
    # (f16p24: dwordx3 granules + one dword per stage and lane — the column scale of the fixed-point operands)
    ldop = ("global_load_dwordx3", "global_load_dword ") if kernel == "f16p24" else ("global_load_dwordx4",)
    hot = [(n, b) for n, b in blocks if sum(1 for x in b if x.startswith("v_mfma")) >= (60 if kernel.startswith("f16") else 90)
           and any(x.startswith(ldop) for x in b)]
    assert len(hot) == 1, [n for n, _ in hot]
    name, blk = hot[0]
    assert any(x.startswith("s_cbranch") and x.endswith(name) for x in blk), "the hot block must loop onto itself"

    def replay(fifo):
        bad, loads, in_asm = [], 0, False
        for t in blk:
            if t.startswith(";;#ASMSTART"):
                in_asm = True
                continue
            if t.startswith(";;#ASMEND"):
                in_asm = False
                continue
            if not t or t[0] in ";.":
                continue
            if t.startswith(ldop):
                assert in_asm, "a compiler-issued load inside the hand-counted loop: " + t
                fifo.append(_vregs(t.split(",")[0]))
                loads += 1
                continue
            if t.startswith("s_waitcnt") and "vmcnt" in t:
                n = int(re.search(r"vmcnt\((\d+)\)", t).group(1))
                while len(fifo) > n:
                    fifo.pop(0)
                continue
            pend = set().union(*fifo) if fifo else set()
            hit = _vregs(t) & pend
            if hit:
                bad.append((t, sorted(hit)))
        return bad, loads

    fifo = []
    bad1, loads = replay(fifo)
    carried = len(fifo)
    bad2, _ = replay(fifo)
    scratch = sum(1 for _, b in blocks for x in b if x.startswith("scratch_"))
    return {"bad": bad1 + bad2, "loads": loads, "carried": carried, "scratch": scratch}


def analyse_f16(asm_path, width=256, family="f16"):
    """fp16x3 sweep kernels (sweep_f16*_kernel in dudf_sweep_bf16.hip).  The order of a step's vector-memory operations
    differs between the two halves of a workgroup and from the bf16x6 kernels (the tail — and its stash stores — may run in
    front of the step's DMA pieces), so the check replays the FIFO instead of comparing against a formula: vmcnt retires in
    issue order, hence at every hand-written `s_waitcnt vmcnt(N)` exactly the N youngest operations may still be in
    flight.  The chunk a step reads after its wait was issued BEFORE the previous hand-written wait: none of those DMA
    pieces may be among the N youngest ("late" pieces).  Returns per kernel {"waits": [(N, late, slack)], "scratch"} where
    slack = how many more operations the wait could have left in flight (0 = as loose as safety allows)."""
    txt = open(asm_path).read()
    out = {}
    # family "f16p": the builds with the 24-bit tile-major stash (sweep_f16p*_kernel: dwordx3 stash accesses, same step structure)
    for m in re.finditer(r"^(_ZN\w*sweep_%s_(?:np_)?kernelILi%dELi(\d)ELi(\d)E\w*):[^\n]*$" % (family, width), txt, re.M):
        body = txt[m.end():txt.index("s_endpgm", m.end())]
        in_asm, scratch, fifo, waits, epoch = False, 0, [], [], 0
        for ln in body.split("\n"):
            t = ln.strip()
            if t.startswith(";;#ASMSTART"):
                in_asm = True
            elif t.startswith(";;#ASMEND"):
                in_asm = False
            if t.startswith("scratch_"):
                scratch += 1
            if t.startswith("global_load_lds"):
                fifo.append(("dma", epoch))
            elif re.match(r"(global_load|global_store|global_atomic|buffer_|flat_)", t):
                fifo.append(("op", epoch))
            elif t.startswith("s_waitcnt") and "vmcnt" in t:
                n = int(re.search(r"vmcnt\((\d+)\)", t).group(1))
                if not in_asm:                       # a compiler wait: retires, never harms
                    fifo = fifo[len(fifo) - n:] if n < len(fifo) else fifo
                    continue
                if n == 0:
                    continue                         # drains (tile start, the stream's last two steps; not-taken branches in
                                                     # the steady state): always safe, and not part of the step sequence
                young = fifo[len(fifo) - n:] if n else []
                late = sum(1 for kind, ep in young if kind == "dma" and ep < epoch)
                # slack: operations older than the N youngest that are NOT old DMA pieces, counted up to the first such piece
                slack = 0
                for kind, ep in reversed(fifo[:len(fifo) - n] if n else fifo):
                    if kind == "dma" and ep < epoch:
                        break
                    slack += 1
                if n:
                    waits.append((n, late, slack))
                fifo = young
                epoch += 1
        # spills INSIDE a block that multiplies (the hand-counted k-block steps) would sit in the vmcnt queue between the DMA
        # pieces; a long-lived scalar parked once at kernel entry and fetched at its exit does not
        # (a k-block step multiplies on the 16-bit cores: v_mfma_f32_16x16x32_*; the output stage of a pass — once per pass, not per
        #  step — uses the f32-input MFMA: a value parked across the whole layer loop and fetched there is `scratch_pass`)
        hot, per_pass, cur, cur_mfma, cur_f32 = 0, 0, 0, False, False
        for ln in body.split("\n") + [".LBB_end:"]:
            t = ln.strip()
            if re.match(r"^\.LBB", t):
                if cur_mfma:
                    hot += cur
                elif cur_f32:
                    per_pass += cur
                cur, cur_mfma, cur_f32 = 0, False, False
            elif t.startswith("scratch_"):
                cur += 1
            elif t.startswith("v_mfma_f32_16x16x32"):
                cur_mfma = True
            elif t.startswith("v_mfma"):
                cur_f32 = True
        out[(int(m.group(2)), int(m.group(3)))] = {"waits": waits, "scratch": scratch, "scratch_hot": hot, "scratch_pass": per_pass}
    return out
