#!/usr/bin/env python3
"""Per-kernel resources and fp32 instruction counts of a device assembly file, for parent-against-new comparisons of a
refactor (profiles/bn_bwd_math_isa.txt).  No GPU is needed:

  hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S csrc/FILE.hip -o FILE.s
  tools/isa_counts.py FILE.s [substring of the demangled kernel name ...]

One line per kernel: VGPRs, SGPRs, scratch bytes, static LDS bytes, instructions, then the counts of OPS."""
import re
import subprocess
import sys

OPS = ("v_fma_f32", "v_fmac_f32", "v_pk_fma_f32", "v_mul_f32", "v_pk_mul_f32", "v_add_f32", "v_pk_add_f32", "v_sub_f32")
META = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")
INSTR = re.compile(r"^\s+(?:[sv]_|ds_|global_|buffer_|flat_|scratch_)")


def kernels(path):
    """-> {mangled name: (body lines, {metadata key: int})} for every .amdhsa kernel of the file."""
    text = open(path).read()
    meta = {}
    for blk in re.split(r"\n  - \.agpr_count:", text)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta[name] = {k: int(re.search(re.escape(k) + r":\s+(\d+)", blk).group(1)) for k in META}
    body = {}
    for name in meta:
        m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end" % re.escape(name), text, re.S | re.M)
        body[name] = [ln for ln in m.group(1).splitlines() if INSTR.match(ln)]
    return {n: (body[n], meta[n]) for n in meta}


def main():
    ks = kernels(sys.argv[1])
    names = sorted(ks)
    plain = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.split("\n")
    print("%-78s %4s %4s %7s %6s %6s  %s" % ("kernel", "VGPR", "SGPR", "scratch", "LDS", "instr", " ".join(o[2:-4] for o in OPS)))
    for name, shown in zip(names, plain):
        shown = re.sub(r"^void |\(.*$", "", shown.replace("(anonymous namespace)::", ""))
        if sys.argv[2:] and not any(s in shown for s in sys.argv[2:]):
            continue
        lines, md = ks[name]
        ops = [sum(1 for ln in lines if ln.split()[0] in (o, o + "_e32", o + "_e64")) for o in OPS]
        print("%-78s %4d %4d %7d %6d %6d  %s" % (shown[:78], *(md[k] for k in META), len(lines),
                                                " ".join("%*d" % (len(o) - 6, c) for o, c in zip(OPS, ops))))


if __name__ == "__main__":
    main()
