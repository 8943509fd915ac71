"""dev tool: what the instruction stream of a solver kernel is made of.  The same machinery as tools/lds_wait_census.py -- ONE kernel
translation unit compiled to gfx950 assembly (device side only, with line tables, no GPU needed), every instruction of the kernel
assigned to the source region its line belongs to -- but counted by class instead of by LDS wait:

    fp64    VALU arithmetic on doubles (v_*_f64, conversions included)
    valu    every other VALU instruction (integer, compares, 32-bit moves of another name)
    mov     v_mov_* / v_cndmask_*
    acc     v_accvgpr_* (copies to and from the AGPR half of the register file: spilled VGPRs)
    lane    v_readlane / v_writelane / v_readfirstlane (spilled SGPRs, wave-uniform values)
    lds     ds_*
    scalar  s_* other than waits and s_nop (ALU, branches, scalar loads)
    wait    s_waitcnt
    nop     s_nop
    other   global / flat / buffer / scratch memory and whatever is left

Classes are formed from opcode prefixes only.  The counts are static: instructions, not executions -- branches that exclude
each other both count, a loop body counts once.  They rank where to look; they are not a prediction of time.

    python tools/issue_census.py [obca_kernel_s5_3_6.hip] [--kernel SUBSTRING] [--csrc DIR] [-- extra hipcc flags]
"""
import argparse
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lds_wait_census as lw  # noqa: E402  (compile_asm, metadata, kernel_body, source_regions, region_of)

CLASSES = ("fp64", "valu", "mov", "acc", "lane", "lds", "scalar", "wait", "nop", "other")


def classify(op):
    if op.startswith("v_accvgpr"):
        return "acc"
    if op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
        return "lane"
    if op.startswith(("v_mov", "v_cndmask")):
        return "mov"
    if op.startswith("v_"):
        return "fp64" if "f64" in op else "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith("s_waitcnt"):
        return "wait"
    if op.startswith("s_nop"):
        return "nop"
    if op.startswith("s_"):
        return "scalar"
    return "other"


def census(asm, body, kernel_file, regions):
    """[(region, {class: count})] in order of first appearance"""
    files = {}
    for ln in asm:
        m = re.match(r'\s*\.file\s+(\d+)\s+(?:"[^"]*"\s+)?"([^"]*)"', ln)
        if m:
            files[int(m.group(1))] = os.path.basename(m.group(2))
    rows, order = {}, []
    cur = "(before the first function)"
    for ln in body:
        s = ln.strip()
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", s)
        if m:
            if files.get(int(m.group(1))) == kernel_file and int(m.group(2)) > 0:
                cur = lw.region_of(regions, int(m.group(2)))
            continue
        if not s or s[0] in ".;" or s.endswith(":"):
            continue
        if cur not in rows:
            rows[cur] = dict.fromkeys(CLASSES, 0)
            order.append(cur)
        rows[cur][classify(s.split()[0])] += 1
    return [(k, rows[k]) for k in order]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("unit", nargs="?", default="obca_kernel_s5_3_6.hip")
    ap.add_argument("--kernel", default="obca_ipm_kernel", help="substring of the kernel to take apart (the largest match)")
    ap.add_argument("--csrc", default=lw.entry.CSRC, help="source directory (e.g. of another checkout, to compare)")
    ap.add_argument("extra", nargs="*", help="further hipcc flags, after --")
    a = ap.parse_args()
    asm = lw.compile_asm(a.csrc, a.unit, a.extra)
    meta = lw.metadata(asm)
    print("unit %s   flags %s" % (a.unit, " ".join(lw.entry.HIPCC_FLAGS + a.extra)))
    for k in meta:
        print("  %-44s vgpr %3d agpr %3d sgpr %3d scratch %5d B  vgpr spills %d  sgpr spills %d" %
              (k["name"], k["vgpr"], k["agpr"], k["sgpr"], k["scratch"], k["vgpr_spills"], k["sgpr_spills"]))
    name = max([k["name"] for k in meta if a.kernel in k["name"]], key=lambda n: len(lw.kernel_body(asm, n)))
    regions = lw.source_regions(os.path.join(a.csrc, "obca_kernel.hip"))
    rows = census(asm, lw.kernel_body(asm, name), "obca_kernel.hip", regions)
    print("kernel %s" % name)
    head = "  %-30s %7s" % ("region", "instr") + "".join(" %7s" % c for c in CLASSES)
    print(head)
    tot = dict.fromkeys(CLASSES, 0)
    for lab, r in rows:
        print("  %-30s %7d" % (lab, sum(r.values())) + "".join(" %7d" % r[c] for c in CLASSES))
        for c in CLASSES:
            tot[c] += r[c]
    n = sum(tot.values())
    print("  %-30s %7d" % ("total", n) + "".join(" %7d" % tot[c] for c in CLASSES))
    print("  %-30s %7s" % ("share of the kernel, %", "") + "".join(" %7.1f" % (100.0 * tot[c] / n) for c in CLASSES))
    body = dict(rows).get("obca_ipm_body")
    if body:
        nb = sum(body.values())
        print("  %-30s %7s" % ("share of obca_ipm_body, %", "") + "".join(" %7.1f" % (100.0 * body[c] / nb) for c in CLASSES))


if __name__ == "__main__":
    main()
