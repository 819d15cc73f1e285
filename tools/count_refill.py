#!/usr/bin/env python3
"""Instruction counts of the REFILL section of the traversal kernels (result flush, ray load, setupRay, classification, replayHint), from the ISA text
of kernels_rt.hip -- the companion of count_visit_loop.py, which counts the node-visit loop.

    hipcc <the flags of massivevoxelraytracing_amd/build.py> --cuda-device-only -S csrc/kernels_rt.hip -o rt.s
    tools/count_refill.py rt.s [kernel-name-substring ...]

Per stream kernel, three lines:
  refill    : the blocks of the outer (depth 1) loop of traceStream that belong to no inner loop = everything a refill event can run outside the visit loop
              (with the blocks without a loop comment between the first of them and the loop header: the result flush, when the compiler rotates it in front of the loop)
  irregular : the blocks of the inner loops that do not hold the stack pop's ds_read_b128 (traceIrregular's walk; rare, listed apart)
  kernel    : the whole-kernel metadata (VGPRs, SGPR spills, scratch, LDS, occupancy, code bytes)
Blocks are told apart by the compiler's own block comments ("in Loop: Header=... Depth=n").  VALU = v_* without v_readlane / v_writelane (the SGPR spill
register's lane traffic, counted as `lane`), SALU = s_* without s_waitcnt / s_nop / branches / scalar loads; `nop` is instructions(wait states)."""
import re
import sys

from count_visit_loop import functions

KERNELS = ["kPtTraceStreamILi0", "kPtTraceStreamILi1", "kPtTraceStreamILi2", "kTraceBatchStreamILi0", "kTraceBatchStreamILi1", "kTraceBatchStreamILi2",
           "kRenderPrimaryStreamILi0", "kRenderPrimaryStreamILi1", "kRenderPrimaryStreamILi2"]
FIELDS = ("total", "valu", "salu", "branch", "saveexec", "nop", "waitcnt", "lds", "vmem", "smem", "lane")


def blocks(lines, a, b):
    """[(first, last, header of the innermost loop the block is in or None, depth)] for every block, fall-through blocks ('; %bb.N:') included"""
    out = []
    for i in range(a, b):
        m = re.match(r"^(?:\.L(BB\d+_\d+):|; %bb\.\d+:)(.*)", lines[i])
        if not m:
            continue
        rest = m.group(2)
        if i + 1 < b and "This" in lines[i + 1] and "Loop Header" in lines[i + 1]:  # "Parent Loop ..." on the label's line, "=> This Inner Loop Header: Depth=n" on the next
            rest += lines[i + 1]
        h = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", rest)
        own = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", rest)
        if own:
            out.append([i, None, m.group(1), int(own.group(1))])
        elif h:
            out.append([i, None, h.group(1), int(h.group(2))])
        else:
            out.append([i, None, None, 0])
    for x, nxt in zip(out, out[1:] + [[b]]):
        x[1] = nxt[0] - 1
    return out


def count(lines, ranges):
    c = dict.fromkeys(FIELDS, 0)
    c["nop_states"] = 0
    for l in (l for lo, hi in ranges for l in lines[lo:hi + 1]):
        m = re.match(r"^\s+([a-z_0-9]+)\b", l)
        if not m or l.lstrip().startswith((".", ";")):
            continue
        op = m.group(1)
        if not re.match(r"^(v_|s_|ds_|global_|flat_|buffer_|scratch_)", op):
            continue
        c["total"] += 1
        if re.match(r"^v_(readlane|writelane)", op):
            c["lane"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
        elif re.match(r"^s_c?branch", op):
            c["branch"] += 1
        elif op == "s_waitcnt":
            c["waitcnt"] += 1
        elif op == "s_nop":
            c["nop"] += 1
            c["nop_states"] += int(re.search(r"s_nop\s+(\d+)", l).group(1)) + 1
        elif re.match(r"^s_(load|buffer_load)", op):
            c["smem"] += 1
        elif op.startswith("s_"):
            c["salu"] += 1
            if "saveexec" in op:
                c["saveexec"] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
        else:
            c["vmem"] += 1
    return c


def metadata(lines, name, b):
    meta = {}
    for l in lines[b:b + 60]:
        m = re.match(r"^;\s*(codeLenInByte|NumVgprs|TotalNumSgprs|ScratchSize|LDSByteSize|Occupancy)\W+(\d+)", l)
        if m:
            meta.setdefault(m.group(1), int(m.group(2)))
    for i, l in enumerate(lines):  # the spill counts are only in the code object's notes
        if l.strip() == ".name:           " + name or re.match(r"^\s*\.name:\s+%s$" % re.escape(name), l):
            for k in lines[i:i + 12]:
                m = re.match(r"^\s*\.(sgpr_spill_count|vgpr_spill_count):\s+(\d+)", k)
                if m:
                    meta[m.group(1)] = int(m.group(2))
    return meta


def fmt(c):
    return "total %4d  VALU %4d  SALU %4d  branches %3d  saveexec %3d  s_nop %3d(%d)  s_waitcnt %3d  LDS %3d  VMEM %3d  smem %3d  lane r/w %3d  | VALU+SALU+s_nop %4d" % (
        c["total"], c["valu"], c["salu"], c["branch"], c["saveexec"], c["nop"], c["nop_states"], c["waitcnt"], c["lds"], c["vmem"], c["smem"], c["lane"],
        c["valu"] + c["salu"] + c["nop"])


def main():
    lines = open(sys.argv[1]).read().split("\n")
    want = sys.argv[2:] or KERNELS
    fns = functions(lines)
    for w in want:
        for name, (a, b) in fns.items():
            if w not in name:
                continue
            bl = blocks(lines, a, b)
            pop = next((i for i in range(a, b) if "ds_read_b128" in lines[i]), None)
            outer = [x for x in bl if x[3] == 1]
            if outer:  # the result flush, rotated in front of the header, carries no loop comment
                header = next(x[0] for x in bl if x[3] == 1 and re.match(r"^\.L%s:" % x[2], lines[x[0]]))
                outer = [x for x in bl if x[3] == 1 or (x[3] == 0 and outer[0][0] <= x[0] < header)]
            if pop is None or not outer:
                print(w, "no stream loop found")
                continue
            visit = next(x[2] for x in bl if x[0] <= pop <= x[1])
            inner = [x for x in bl if x[3] >= 2 and x[2] != visit]
            # a depth-3 block names its depth-2 header: blocks of loops nested in the visit loop stay with the visit loop
            nested_in_visit = {x[2] for x in bl if x[3] >= 3 and any(v[2] == visit and v[0] < x[0] < max(y[1] for y in bl if y[2] == visit) for v in bl)}
            inner = [x for x in inner if x[2] not in nested_in_visit]
            print("%-26s refill    %s" % (w, fmt(count(lines, [(x[0], x[1]) for x in outer]))))
            print("%-26s irregular %s" % ("", fmt(count(lines, [(x[0], x[1]) for x in inner]))))
            print("%-26s kernel    %s" % ("", "  ".join("%s %d" % kv for kv in sorted(metadata(lines, name, b).items()))))


if __name__ == "__main__":
    main()
