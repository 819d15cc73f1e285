#!/usr/bin/env python3
"""usage: tools/combine_bench.py [--scenes dragon[:grid],tunnel[:grid]] [--ops listing,inplace] [--reps 5] [--warmup 1] [--host-reps 2] [--shift 8] [--step-timeout 420]
                                 [--out profiles/combine_bench.json]

Cost of the two-set calls on the procedural stand-ins (dragon 2048^3, tunnel 4096^3), b being a second build of the same model, per scene:
  listing   combine_count / combine_list   mvrt_svo_combine_voxels, the sizing call and the listing of all three arrays into device arrays, for every op, with a
                                           zero offset (b's codes as they are: no translate, no sort) and with b moved by --shift cells along x (translate,
                                           compact, radix sort).  The difference between the two rows of an op is the cost of that stage; that the zero-offset
                                           path skips it shows in nothing but this timing.
  inplace   combine                        mvrt_svo_combine with b moved by --shift cells, every op
            host_route                     the same change by the route that exists without the call: mvrt_svo_read_voxels of both handles to the host, the set
                                           operation in numpy on linear cell keys, the added and the dropped voxels back through mvrt_svo_edit_voxels
The octree is rebuilt from its voxel list before every timed in-place call, outside the clock.  Median of --reps calls after --warmup calls (host_route:
--host-reps calls, no warm-up: seconds each); host clock around each call (every call blocks).  A call the library refuses is reported with its message, never
guessed.  MVRT_LIB in the environment selects another build of the library (an A/B of two kernels); a kernel trace of one step is taken by running
`--step scene:grid:op` under the profiler, in a run of its own.
Every step runs in a child process of its own under --step-timeout seconds; a step that fails, is killed or runs out of time ends the run: nothing more is
started on the GPU behind it."""
import argparse
import os
import sys

import numpy as np

import benchkit as bk

OPS = {"union": 0, "intersection": 1, "difference": 2, "xor": 3}


def keys_of(xyz, res):
    x = xyz.astype(np.uint64)
    return (x[:, 2] * np.uint64(res) + x[:, 1]) * np.uint64(res) + x[:, 0]


def host_route(svo, b, op, offset, res):
    """read both lists, combine on the host, edit: what a caller does without mvrt_svo_combine"""
    (xa, _), (xb, ab) = svo.read_voxels(), b.read_voxels()
    moved = xb.astype(np.int64) + np.asarray(offset, np.int64)
    inside = ((moved >= 0) & (moved < res)).all(1)
    xb, ab = moved[inside].astype(np.uint32), ab[inside]
    ka, kb = keys_of(xa, res), keys_of(xb, res)
    a_in_b = np.isin(ka, kb, assume_unique=True)
    b_in_a = np.isin(kb, ka, assume_unique=True)
    add = ~b_in_a if op in (OPS["union"], OPS["xor"]) else np.zeros(len(kb), bool)
    drop = {OPS["union"]: np.zeros(len(ka), bool), OPS["intersection"]: ~a_in_b, OPS["difference"]: a_in_b, OPS["xor"]: a_in_b}[op]
    xyz = np.concatenate([xb[add], xa[drop]])
    if len(xyz):
        svo.edit_voxels(xyz, np.concatenate([ab[add], np.zeros((int(drop.sum()), 8), np.uint8)]),
                        np.concatenate([np.ones(int(add.sum()), np.uint8), np.zeros(int(drop.sum()), np.uint8)]))
    return [int(add.sum()), int(drop.sum()), int((~inside).sum())]


def step(args):
    """one child process: prints one JSON row per measurement"""
    import massivevoxelraytracing_amd as mv
    mv.set_device(0)
    name, res, what = args.step.split(":")
    res = int(res)
    svo, origin, dps = bk.built(mv, name, res)
    b, _, _ = bk.built(mv, name, res)
    base = dict(scene=name, grid=res, voxels=svo.info().numberOfVoxels, lib=os.path.basename(mv.LIB_PATH))

    def measure(label, fn, before=None, reps=args.reps, warmup=args.warmup, **kw):
        return bk.timed_or_refused(mv, base, label, fn, reps, warmup, before, **kw)

    shifted = (args.shift, 0, 0)
    if what == "listing":
        for oname, op in OPS.items():
            for offset in ((0, 0, 0), shifted):
                got = measure("combine_count", lambda: list(svo.combine_voxels_device(b, op, offset)), set_op=oname, offset=list(offset))
                if got and got[0]:
                    n = got[0]
                    xyz, at, src = mv.DeviceArray((n, 3), np.uint32), mv.DeviceArray((n, 8), np.uint8), mv.DeviceArray(n, np.uint8)
                    measure("combine_list", lambda: list(svo.combine_voxels_device(b, op, offset, 0, n, xyz, at, src)), set_op=oname, offset=list(offset))
                    del xyz, at, src
    elif what == "inplace":
        original = bk.snapshot(mv, svo)

        def restore():
            svo.build_voxels(original[0], original[1], origin=origin, dps=dps, gridRes=res)

        for oname, op in OPS.items():
            measure("combine", lambda: list(svo.combine(b, op, shifted)), before=restore, set_op=oname, offset=list(shifted))
            measure("host_route", lambda: host_route(svo, b, op, shifted, res), before=restore, reps=args.host_reps, warmup=0, set_op=oname, offset=list(shifted))


def line(r):
    what = "%9.2f ms" % r["ms"] if "ms" in r else r.get("refused") or r.get("failed")
    return "%-7s %5s %-12s %-14s %-10s %10s voxels  %s  -> %s" % (r.get("scene", r.get("step")), r.get("grid", ""), r.get("set_op", ""), r.get("op", ""),
                                                                 r.get("offset", ""), r.get("voxels", ""), what, r.get("result", ""))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=bk.parse_scenes, default="dragon,tunnel")
    ap.add_argument("--ops", default="listing,inplace")
    ap.add_argument("--shift", type=int, default=8)
    ap.add_argument("--host-reps", type=int, default=2)
    bk.add_step_args(ap, reps=5, warmup=1, step_timeout=420)
    args = ap.parse_args()
    if args.step:
        return step(args)
    steps = ["%s:%d:%s" % (name, res, op) for name, res in args.scenes for op in args.ops.split(",")]
    rows, rc = bk.run_steps(__file__, steps, lambda s: bk.flags(args, "reps", "warmup", "host_reps", "shift"), args.step_timeout, args.out)
    bk.print_table(rows, line)
    return rc


if __name__ == "__main__":
    sys.exit(main())
