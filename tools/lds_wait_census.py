"""dev tool: where the LDS waits of a solver kernel sit.  Compiles ONE kernel translation unit to gfx950 assembly (device side
only, with line tables, no GPU needed), assigns every instruction of the kernel to the source region its line belongs to -- a
function of csrc/obca_kernel.hip, riccati() further split at its phase comments -- and prints per region
    LDS ops | lgkm waits | waits right behind their load | scratch instructions
where "right behind" means: at most two VALU instructions between the wait and the LDS operation it waits for (LDS
operations complete in order, so `s_waitcnt lgkmcnt(n)` waits for the (n+1)-th last one).  With one wavefront per SIMD nothing
covers such a wait.  The counts are static: instructions, not executions, and branches that exclude each other both count.
Registers, scratch and spill counts of every kernel in the unit come from the code-object metadata in the same assembly.

    python tools/lds_wait_census.py [obca_kernel_s5_3_6.hip] [--kernel SUBSTRING] [--csrc DIR] [-- extra hipcc flags]
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402  (the product's compile flags)

# riccati() is split where these comments stand (first match at or after the function's first line)
RICCATI_MARKS = (("---- phase A", "riccati: phase A"), ("---- phase B", "riccati: phase B"), ("// stage 0:", "riccati: stage 0"),
                 ("---- forward pass", "riccati: forward pass"), ("// local recovery", "riccati: local recovery"))
DEF = re.compile(r"^(?:template\s*<[^>]*>\s*)?(?:static\s+)?(?:__device__|__global__)\b[^;{]*?\b([A-Za-z_]\w*)\s*\(")


def source_regions(path):
    """[(first line, label)] sorted by line: every function definition at column 0, riccati split at its marks"""
    out, in_riccati, marks = [], False, []
    with open(path) as f:
        lines = f.read().split("\n")
    for no, text in enumerate(lines, 1):
        m = DEF.match(text)
        if m and not text.rstrip().endswith(";"):
            name = m.group(1)
            if out and out[-1][1] == name:      # the two signatures of riccati (#ifdef OBCA_PROFILE)
                continue
            out.append((no, name))
            in_riccati = name == "riccati"
            marks = list(RICCATI_MARKS)
        elif in_riccati and marks and marks[0][0] in text:
            out.append((no, marks.pop(0)[1]))
    return out


def region_of(regions, line):
    lab = "(before the first function)"
    for no, name in regions:
        if no > line:
            break
        lab = name
    return lab


def compile_asm(csrc, unit, extra):
    tmp = tempfile.mkdtemp(prefix="lds_census_")
    out = os.path.join(tmp, "unit.s")
    cmd = ["hipcc"] + entry.HIPCC_FLAGS + extra + ["-gline-tables-only", "-S", "--cuda-device-only", os.path.join(csrc, unit), "-o", out]
    subprocess.run(cmd, check=True, cwd=csrc)
    with open(out) as f:
        return f.read().split("\n")


def metadata(asm):
    """register / scratch figures per kernel from the amdhsa.kernels notes at the end of the assembly"""
    txt = "\n".join(asm)
    recs = []
    for blk in txt.split("- .agpr_count:")[1:]:
        g = lambda k: re.search(r"\.%s:\s+(\S+)" % k, blk)
        recs.append(dict(name=g("name").group(1), agpr=int(blk.split()[0]), vgpr=int(g("vgpr_count").group(1)), sgpr=int(g("sgpr_count").group(1)),
                         scratch=int(g("private_segment_fixed_size").group(1)), vgpr_spills=int(g("vgpr_spill_count").group(1)),
                         sgpr_spills=int(g("sgpr_spill_count").group(1))))
    return recs


def kernel_body(asm, name):
    start = next(i for i, ln in enumerate(asm) if ln.startswith(name + ":"))
    end = next(i for i in range(start, len(asm)) if asm[i].startswith(".Lfunc_end"))
    return asm[start + 1:end]


def census(asm, body, kernel_file, regions):
    files = {}
    for ln in asm:
        m = re.match(r'\s*\.file\s+(\d+)\s+(?:"[^"]*"\s+)?"([^"]*)"', ln)
        if m:
            files[int(m.group(1))] = os.path.basename(m.group(2))
    rows, order = {}, []
    cur = "(before the first function)"
    hist = []                       # instructions so far: "lds" | "valu" | "other"
    for ln in body:
        s = ln.strip()
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", s)
        if m:
            if files.get(int(m.group(1))) == kernel_file and int(m.group(2)) > 0:
                cur = region_of(regions, int(m.group(2)))
            continue
        if not s or s[0] in ".;" or s.endswith(":"):
            continue
        op = s.split()[0]
        if cur not in rows:
            rows[cur] = dict(lds=0, waits=0, tight=0, scratch=0)
            order.append(cur)
        r = rows[cur]
        if op.startswith("ds_"):
            r["lds"] += 1
            hist.append("lds")
        elif op.startswith("scratch_") or (op.startswith("buffer_") and "offen" in s and "s[0:3]" in s):
            r["scratch"] += 1
            hist.append("other")
        elif op == "s_waitcnt" and "lgkmcnt" in s:
            n = int(re.search(r"lgkmcnt\((\d+)\)", s).group(1))
            r["waits"] += 1
            seen, valu = 0, 0
            for h in reversed(hist):
                if h == "lds":
                    seen += 1
                    if seen == n + 1:
                        r["tight"] += valu <= 2
                        break
                elif h == "valu":
                    valu += 1
                    if valu > 2:
                        break
            hist.append("other")
        else:
            hist.append("valu" if op.startswith("v_") else "other")
    return [(k, rows[k]) for k in order]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("unit", nargs="?", default="obca_kernel_s5_3_6.hip")
    ap.add_argument("--kernel", default="obca_ipm_kernel", help="substring of the kernel to take apart (the largest match)")
    ap.add_argument("--csrc", default=entry.CSRC, help="source directory (e.g. of another checkout, to compare)")
    ap.add_argument("extra", nargs="*", help="further hipcc flags, after --")
    a = ap.parse_args()
    asm = compile_asm(a.csrc, a.unit, a.extra)
    meta = metadata(asm)
    print("unit %s   flags %s" % (a.unit, " ".join(entry.HIPCC_FLAGS + a.extra)))
    for k in meta:
        print("  %-44s vgpr %3d agpr %3d sgpr %3d scratch %5d B  vgpr spills %d  sgpr spills %d" %
              (k["name"], k["vgpr"], k["agpr"], k["sgpr"], k["scratch"], k["vgpr_spills"], k["sgpr_spills"]))
    cands = [k["name"] for k in meta if a.kernel in k["name"]]
    name = max(cands, key=lambda n: len(kernel_body(asm, n)))
    regions = source_regions(os.path.join(a.csrc, "obca_kernel.hip"))
    rows = census(asm, kernel_body(asm, name), "obca_kernel.hip", regions)
    print("kernel %s" % name)
    print("  %-34s %8s %11s %13s %8s" % ("region", "LDS ops", "lgkm waits", "right behind", "scratch"))
    tot = dict(lds=0, waits=0, tight=0, scratch=0)
    for lab, r in rows:
        print("  %-34s %8d %11d %13d %8d" % (lab, r["lds"], r["waits"], r["tight"], r["scratch"]))
        for k in tot:
            tot[k] += r[k]
    print("  %-34s %8d %11d %13d %8d" % ("total", tot["lds"], tot["waits"], tot["tight"], tot["scratch"]))


if __name__ == "__main__":
    main()
