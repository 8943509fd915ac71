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

With --frames a second table follows: the divergent-branch frames of the kernel.  A frame opens at an instruction that saves
the execution mask into a scalar register pair while narrowing it (s_and_saveexec / s_andn2_saveexec: any s_*_saveexec), and
closes at the first later scalar instruction that writes exec and reads that pair -- in the order of the assembly text, nested
frames included in their parents.  Per frame: the source line and region of the save, the s_cbranch_exec* that follows the
save directly (the skip over the body, if the compiler kept one), and the instructions between save and restore by class --
valu (fp64 + valu + mov), copies (acc + lane), lds, scalar, other (memory).  A frame whose pair is spilled and comes back in
another register never closes here: it is counted as open and not listed.  Listed are the closed frames with at most MAX_VALU
VALU instructions and no LDS or memory instruction -- what a select can replace -- and the
number of frames and of such short ones per region.

Classes are formed from opcode prefixes only.  The counts are static: instructions, not executions -- branches that exclude
each other both count, a loop body counts once.  They rank where to look; they are not a prediction of time.

    python tools/issue_census.py [obca_kernel_s5_3_6.hip] [--kernel SUBSTRING] [--csrc DIR] [--frames [MAX_VALU]] [-- extra hipcc flags]
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


def file_table(asm):
    """{file number of the line tables: base name}"""
    files = {}
    for ln in asm:
        m = re.match(r'\s*\.file\s+(\d+)\s+(?:"[^"]*"\s+)?"([^"]*)"', ln)
        if m:
            files[int(m.group(1))] = os.path.basename(m.group(2))
    return files


def census(asm, body, kernel_file, regions):
    """[(region, {class: count})] in order of first appearance"""
    files = file_table(asm)
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


FRAME_COLS = ("valu", "copies", "lds", "scalar", "other")
_FRAME_COL = {"fp64": "valu", "valu": "valu", "mov": "valu", "acc": "copies", "lane": "copies", "lds": "lds", "scalar": "scalar",
              "wait": None, "nop": None, "other": "other"}


def _operands(s):
    return [t.strip() for t in s.split(None, 1)[1].split(",")] if " " in s.strip() else []


def frames(body, files=None, kernel_file=None, regions=None):
    """[{line, region, op, branch, closed, valu, copies, lds, scalar, other}] in the order of the saves.  ``files`` / ``kernel_file``
    / ``regions`` as in census(); without them every .loc line counts and the region is None."""
    out, live = [], []
    line = 0
    prev_save = None                      # the frame whose save was the previous instruction (its branch may follow)
    for ln in body:
        s = ln.strip()
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", s)
        if m:
            if int(m.group(2)) > 0 and (files is None or files.get(int(m.group(1))) == kernel_file):
                line = int(m.group(2))
            continue
        if not s or s[0] in ".;" or s.endswith(":"):
            continue
        s = s.split(";")[0].strip()
        op, ops = s.split()[0], _operands(s)
        own = prev_save if op.startswith("s_cbranch_exec") else None       # the skip over the body belongs to the frame, not to its body
        if own is not None:
            own["branch"] = op
        prev_save = None
        if op.startswith("s_") and ops and ops[0] == "exec" and live:
            for f in [f for f in live if f["_pair"] in ops[1:]]:
                f["closed"] = True
                live.remove(f)
        col = _FRAME_COL[classify(op)]
        if col:
            for f in live:
                if f is not own:
                    f[col] += 1
        if op.startswith("s_") and "saveexec" in op and ops:
            f = dict(line=line, region=lw.region_of(regions, line) if regions else None, op=op, branch=None, closed=False, _pair=ops[0])
            f.update(dict.fromkeys(FRAME_COLS, 0))
            out.append(f)
            live.append(f)
            prev_save = f
    for f in out:
        del f["_pair"]
    return out


def print_frames(fr, max_valu):
    print("frames: %d, closed %d; listed: closed, at most %d valu, no lds / other" % (len(fr), sum(f["closed"] for f in fr), max_valu))
    print("  %-30s %6s %-22s %-18s" % ("region", "line", "save", "branch") + "".join(" %7s" % c for c in FRAME_COLS))
    per = {}
    for f in fr:
        short = f["closed"] and f["valu"] <= max_valu and not f["lds"] and not f["other"]
        k = per.setdefault(f["region"], [0, 0])
        k[0] += 1
        k[1] += short
        if short:
            print("  %-30s %6d %-22s %-18s" % (f["region"], f["line"], f["op"], f["branch"] or "-") + "".join(" %7d" % f[c] for c in FRAME_COLS))
    print("  per region: frames / short ones")
    for r, (n, k) in per.items():
        print("  %-30s %6d %6d" % (r, n, k))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("unit", nargs="?", default="obca_kernel_s5_3_6.hip")
    ap.add_argument("--kernel", default="obca_ipm_kernel", help="substring of the kernel to take apart (the largest match)")
    ap.add_argument("--csrc", default=lw.entry.CSRC, help="source directory (e.g. of another checkout, to compare)")
    ap.add_argument("--frames", nargs="?", type=int, const=6, default=None, metavar="MAX_VALU",
                    help="also list the divergent-branch frames whose body holds at most MAX_VALU (6) VALU instructions")
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
    kbody = lw.kernel_body(asm, name)
    rows = census(asm, kbody, "obca_kernel.hip", regions)
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
    if a.frames is not None:
        print_frames(frames(kbody, file_table(asm), "obca_kernel.hip", regions), a.frames)


if __name__ == "__main__":
    main()
