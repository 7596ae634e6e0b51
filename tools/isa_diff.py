#!/usr/bin/env python3
"""Compare the kernels of two builds of the same libraries, instruction for instruction.

  python tools/isa_diff.py OLD_DIR NEW_DIR [library.so ...] [-o table.txt]

For every kernel of every named library (default: all libos2r*.so found in OLD_DIR) the disassembly of both builds is
normalised (addresses dropped; branch targets are already relative) and compared.  One line per kernel: identical or not, and where
not, the delta of the instruction-class histogram (the classes of isa_histogram.py), of every floating-point and conversion
mnemonic (whatever its encoding: _e32 and _e64 count as one), and of the metadata fields that say what the kernel occupies.  Exit status 1 if a kernel differs in a floating-point
or conversion count, in LDS size, or in more scratch, VGPR spills or AGPRs than before; 0 otherwise.  Static: what the code objects hold.
"""
import argparse
import collections
import glob
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_histogram import classify, disassemble_all   # noqa: E402
from kernel_meta import kernel_meta                    # noqa: E402

META = ("vgpr_count", "agpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count", "group_segment_fixed_size", "private_segment_fixed_size")
MUST_NOT_GROW = ("agpr_count", "vgpr_spill_count", "private_segment_fixed_size")
FLOAT = re.compile(r"^v_cvt|_(f16|bf16|f32|f64)(_|$)")


def kernels(path):
    """{demangled kernel name: [(mnemonic, operands)]}: addresses dropped, the symbol a branch target is relative to left out"""
    return {name: [(mn, re.sub(r"<[^>+]*\+", "<+", ops)) for _, mn, ops in insts] for name, insts in disassemble_all(path).items()}


def float_counts(insts):
    """every floating-point or conversion mnemonic, its encoding suffix (_e32, _e64, ...) dropped, -> its count"""
    return collections.Counter(re.sub(r"_(e32|e64|dpp|sdwa)$", "", m) for m, _ in insts if FLOAT.search(m))


def delta(a, b):
    return {k: b.get(k, 0) - a.get(k, 0) for k in sorted(set(a) | set(b)) if a.get(k, 0) != b.get(k, 0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("libs", nargs="*")
    ap.add_argument("-o", "--out", default=None)
    a = ap.parse_args()
    libs = a.libs or sorted(os.path.basename(p) for p in glob.glob(os.path.join(a.old, "libos2r*.so")))
    lines, bad, total, same = [], 0, 0, 0
    for lib in libs:
        old, new = os.path.join(a.old, lib), os.path.join(a.new, lib)
        ko, kn, mo, mn = kernels(old), kernels(new), kernel_meta(old), kernel_meta(new)
        lines.append(f"{lib}: {len(ko)} kernels before, {len(kn)} after")
        for name in sorted(set(ko) | set(kn)):
            total += 1
            if name not in ko or name not in kn:
                lines.append(f"  MISSING {'before' if name not in ko else 'after'}  {name}")
                bad += 1
                continue
            io, inw = ko[name], kn[name]
            o, n = mo.get(name, {}), mn.get(name, {})
            dmeta = {f: (o.get(f), n.get(f)) for f in META if o.get(f) != n.get(f)}
            dfloat = delta(float_counts(io), float_counts(inw))
            hard = bool(dfloat) or "group_segment_fixed_size" in dmeta or any((n.get(f) or 0) > (o.get(f) or 0) for f in MUST_NOT_GROW)
            bad += hard
            if io == inw and not dmeta:
                same += 1
                lines.append(f"  identical ({len(io)} instructions)  {name}")
                continue
            lines.append(f"  {'DIFFERS, HARD CONDITION BROKEN' if hard else 'differs'} ({len(io)} -> {len(inw)} instructions)  {name}")
            lines.append(f"      classes  {delta(collections.Counter(classify(m) for m, _ in io), collections.Counter(classify(m) for m, _ in inw))}")
            lines.append(f"      float / conversion  {dfloat or 'identical counts'}")
            lines.append(f"      metadata (before, after)  {dmeta or 'identical'}")
    lines.append(f"{same} of {total} kernels identical; {bad} break a hard condition (float / conversion counts, LDS, scratch, spills, AGPRs)")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        open(a.out, "w").write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
