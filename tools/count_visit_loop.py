#!/usr/bin/env python3
"""Instruction counts of the node-visit loop of the traversal kernels, from the ISA text of kernels_rt.hip.

    hipcc <the flags of massivevoxelraytracing_amd/build.py> --cuda-device-only -S csrc/kernels_rt.hip -o rt.s
    tools/count_visit_loop.py rt.s [kernel-name-substring ...]

The visit loop of a kernel = the smallest backward-branch range (loop header label .. back edge) that holds the stack pop's
ds_read_b128; rare blocks the compiler lays out inside that range (the ring eviction) are counted with it.  VALU = v_*,
SALU = s_* without s_waitcnt / s_nop / branches / scalar memory loads, as in profiles/r10_traversal_diet.txt."""
import re
import sys

KERNELS = ["kPtTraceStreamILi0", "kPtTraceStreamILi1", "kPtTraceStreamILi2", "kTraceBatchStreamILi0", "kTraceBatchStreamILi1", "kTraceBatchStreamILi2"]


def functions(lines):
    """name -> (first, last) line index of the function body"""
    out, name, start = {}, None, 0
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z\w+):", l)
        if m:
            name, start = m.group(1), i
        elif name and l.startswith(".Lfunc_end"):
            out[name] = (start, i)
            name = None
    return out


def visit_loop(lines, a, b):
    """the blocks of the innermost loop around the pop, by the compiler's own block comments: [(first, last)]"""
    blocks = []  # (label, first line, header named in the comment or None)
    for i in range(a, b):
        m = re.match(r"^\.L(BB\d+_\d+):(.*)", lines[i])
        if m:
            h = re.search(r"Header[=:]\s*(BB\d+_\d+)", m.group(2))
            blocks.append((m.group(1), i, h.group(1) if h else None, "Loop Header" in m.group(2) or "Parent Loop" in m.group(2)))
    ends = [x[1] for x in blocks[1:]] + [b]
    pop = next((i for i in range(a, b) if "ds_read_b128" in lines[i]), None)
    if pop is None:
        return None
    k = max(j for j, x in enumerate(blocks) if x[1] < pop)
    header = blocks[k][2] if blocks[k][2] else blocks[k][0]
    if blocks[k][3] and not blocks[k][2]:
        header = blocks[k][0]
    return [(x[1], e - 1) for x, e in zip(blocks, ends) if x[0] == header or x[2] == header]


def count(lines, ranges):
    c = dict(total=0, valu=0, salu=0, branch=0, smem=0, vmem_lds=0, other=0)
    for l in (l for lo, hi in ranges for l in lines[lo:hi + 1]):
        m = re.match(r"^\s+([a-z_0-9]+)\b", l)
        if not m or l.lstrip().startswith((".", ";")):
            continue
        op = m.group(1)
        if not re.match(r"^(v_|s_|ds_|global_|flat_|buffer_|scratch_)", op):
            continue
        c["total"] += 1
        if op.startswith("v_"):
            c["valu"] += 1
        elif re.match(r"^s_c?branch", op):
            c["branch"] += 1
        elif op in ("s_waitcnt", "s_nop"):
            c["other"] += 1
        elif re.match(r"^s_(load|buffer_load)", op):
            c["smem"] += 1
        elif op.startswith("s_"):
            c["salu"] += 1
        else:
            c["vmem_lds"] += 1
    return c


def main():
    lines = open(sys.argv[1]).read().split("\n")
    want = sys.argv[2:] or KERNELS
    fns = functions(lines)
    for w in want:
        for name, (a, b) in fns.items():
            if w in name:
                r = visit_loop(lines, a, b)
                if r is None:
                    print(w, "no visit loop found")
                    continue
                c = count(lines, r)
                regs = {}
                for l in lines[b:b + 80]:
                    m = re.match(r"^\s*[;.]\s*\.?(NumVgprs|NumSgprs|sgpr_spill_count|vgpr_spill_count|SGPRBlocks|Occupancy|ScratchSize)\W+(\d+)", l)
                    if m:
                        regs.setdefault(m.group(1), m.group(2))
                print("%-24s lines %d-%d  total %d  VALU %d  SALU %d  branches %d  smem %d  vmem+lds %d  waitcnt/nop %d  %s" % (
                    w, min(x[0] for x in r) + 1, max(x[1] for x in r) + 1, c["total"], c["valu"], c["salu"], c["branch"], c["smem"], c["vmem_lds"], c["other"], regs))


if __name__ == "__main__":
    main()
