#!/usr/bin/env python
"""Per-kernel comparison of two device assemblies of one source file (a host-only refactor must leave every kernel as it was):
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off --cuda-device-only -S FILE.hip -o FILE.s      (both trees)
    python scripts/kernel_isa_diff.py PARENT.s RESULT.s [PARENT2.s RESULT2.s ...] > profiles/NAME.txt
For every kernel: the instruction stream (comments dropped, local label numbers and the kernel's own name normalised) and the
.amdhsa_ resource block (VGPRs, SGPRs, scratch, LDS, ...) must be equal.  A kernel whose mangled name is missing on the other side is
paired by its plain identifier (a kernel that lost a template parameter).  Exit status 1 if anything differs or stays unpaired."""
import re
import sys


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M):
        name, block = m.group(1), m.group(2)
        body = re.search(r"^%s:[^\n]*\n(.*?)^\s*\.amdhsa_kernel %s\n" % (re.escape(name), re.escape(name)), text, re.S | re.M).group(1)
        lines = []
        for line in body.split("\n"):
            line = line.split(";")[0].strip().replace(name, "@K")
            if line:
                lines.append(re.sub(r"\.LBB\d+_", ".LBB_", line))
        res = sorted(l.split(";")[0].strip().replace(name, "@K") for l in block.split("\n") if l.strip())
        out[name] = (lines, res)
    return out


def ident(name):
    m = re.match(r"_Z(\d+)", name)
    return name[m.end():m.end() + int(m.group(1))] if m else name


def field(res, key):
    return next((l.split()[-1] for l in res if l.startswith(".amdhsa_" + key + " ")), "-")


bad = 0
for pa, pb in zip(sys.argv[1::2], sys.argv[2::2]):
    a, b = kernels(pa), kernels(pb)
    print("%s (%d kernels) against %s (%d kernels)" % (pa.split("/")[-1], len(a), pb.split("/")[-1], len(b)))
    for name in sorted(a):
        other = name if name in b else next((n for n in b if n not in a and ident(n) == ident(name)), None)
        if other is None:
            print("  UNPAIRED   %s" % name)
            bad += 1
            continue
        same_i, same_r = a[name][0] == b[other][0], a[name][1] == b[other][1]
        bad += not (same_i and same_r)
        r = a[name][1]
        print("  %-10s %s%s: %d instructions and labels, vgpr %s agpr-offset %s sgpr %s scratch %s lds %s" % (
            "identical" if same_i and same_r else "DIFFERS" + (" isa" if not same_i else "") + (" resources" if not same_r else ""), name,
            "" if other == name else " -> " + other, len(a[name][0]), field(r, "next_free_vgpr"), field(r, "accum_offset"), field(r, "next_free_sgpr"),
            field(r, "private_segment_fixed_size"), field(r, "group_segment_fixed_size")))
    for name in sorted(n for n in b if n not in a and not any(ident(n) == ident(m) and m not in b for m in a)):
        print("  NEW        %s" % name)
        bad += 1
print("%d kernels differ or are unpaired" % bad)
sys.exit(1 if bad else 0)
