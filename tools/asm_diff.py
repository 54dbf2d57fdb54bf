# coding: utf-8
"""Is the device code of two builds of a translation unit the same?  Compares two device-assembly files (hipcc -S
--cuda-device-only, the flags of tests/isa_contract.py::emit_asm) kernel by kernel:
  * the sets of kernel symbols must be equal;
  * per kernel, the instruction stream from the entry label to the end of the function, with basic-block labels (.LBBn_m: the
    function index n moves when the instantiation order does; likewise the `%=` serial numbers of the labels inside inline
    assembly, .Ldudf_poll<n> ...) replaced by their order of appearance and comments dropped;
  * per kernel, the .amdhsa_* descriptor lines (VGPRs, SGPRs, LDS, scratch ...).
    python tools/asm_diff.py OLD.s NEW.s            prints `<kernels compared> kernels, <differences> differences`, exit 1 on any
    python tools/asm_diff.py --emit SRC.hip OUT.s   writes the assembly of one source file"""
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))


def kernels(path):
    txt = open(path).read()
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", txt, re.M | re.S):
        name = m.group(1)
        desc = [ln.strip() for ln in m.group(2).split("\n") if ln.strip().startswith(".amdhsa_")]
        start = re.search(r"^%s:[^\n]*\n" % re.escape(name), txt, re.M)
        end = re.compile(r"^\.Lfunc_end\d+:", re.M).search(txt, start.end())
        labels, body = {}, []
        for ln in txt[start.end():end.start()].split("\n"):
            ln = ln.split(";")[0].strip() if not ln.strip().startswith(";;#ASM") else ln.strip()
            if ln:
                body.append(re.sub(r"(\.L[A-Za-z_]+?)\d+(_\d+)?\b", lambda l: labels.setdefault(l.group(0), "%s#%d" % (l.group(1), len(labels))), ln))
        out[name] = (body, desc)
    return out


def main(old, new):
    a, b = kernels(old), kernels(new)
    diffs = ["only in %s: %s" % (p, k) for p, ks in ((old, set(a) - set(b)), (new, set(b) - set(a))) for k in sorted(ks)]
    for k in sorted(set(a) & set(b)):
        if a[k][0] != b[k][0]:
            diffs.append("instructions differ: " + k)
        if a[k][1] != b[k][1]:
            diffs.append("descriptor differs: " + k)
    print("\n".join(diffs + ["%s: %d kernels, %d differences" % (os.path.basename(new), len(set(a) & set(b)), len(diffs))]))
    return 1 if diffs else 0


if __name__ == "__main__":
    if sys.argv[1] == "--emit":
        from isa_contract import emit_asm
        emit_asm(sys.argv[2], sys.argv[3])
        sys.exit(0)
    sys.exit(main(sys.argv[1], sys.argv[2]))
