#!/usr/bin/env python3
"""usage: tools/morph_bench.py [--scenes dragon[:grid],tunnel[:grid]] [--reps 5] [--warmup 1] [--step-timeout 360] [--close-steps 1,2,4] [--out profiles/morph_bench.json]

Cost of the morphology calls on the procedural stand-ins (dragon 2048^3, tunnel 4096^3), per scene and structuring element (faces, cube):
  dilation_count / dilation_list   mvrt_svo_dilation_cells, the sizing call and the listing into device arrays
  erosion_count / erosion_list     mvrt_svo_erosion_voxels likewise
  dilate1                          mvrt_svo_dilate, one step, on the octree as built
  erode1                           mvrt_svo_erode, one step, on the octree dilated by one step (the scenes are one-voxel shells: their own erosion is empty)
  close{1,2,4}                     mvrt_svo_close with k steps in ONE call: the levels are built once
  close{1,2,4}_steps               the same closing as 2k one-step calls (k x dilate 1, k x erode 1): the levels are built 2k times
  list_edit                        the route through the listing: mvrt_svo_dilation_cells into device arrays + mvrt_svo_edit_voxels
The octree is rebuilt from its own voxel list before every timed call, outside the clock; the one-call closing and its step sequence alternate inside one
process, so that both see the same machine.  Median of --reps calls after --warmup calls; host clock around each call (every call blocks).  A call the library
refuses is reported with its message, never guessed.
Every step runs in a child process of its own under --step-timeout seconds; a step that fails, is killed or runs out of time ends the run: nothing more is
started on the GPU behind it."""
import argparse
import sys

import numpy as np

import benchkit as bk

ELEMENT = {"faces": 0, "cube": 1}


def step(args):
    """one child process: prints one JSON row per measurement"""
    import massivevoxelraytracing_amd as mv
    mv.set_device(0)
    name, res, op, ename = args.step.split(":")
    e, res = ELEMENT[ename], int(res)
    svo, origin, dps = bk.built(mv, name, res)
    n_vox = svo.info().numberOfVoxels
    base = dict(scene=name, grid=res, voxels=n_vox, element=ename)
    as_built = bk.snapshot(mv, svo)

    def restore(list_=as_built):
        svo.build_voxels(list_[0], list_[1], origin=origin, dps=dps, gridRes=res)

    def measure(label, fn, before=None, **kw):
        return bk.timed_or_refused(mv, base, label, fn, args.reps, args.warmup, before, **kw)

    if op == "listings":
        n = measure("dilation_count", lambda: svo.dilation_cells_device(e))
        if n:
            xyz, at, cnt = mv.DeviceArray((n, 3), np.uint32), mv.DeviceArray((n, 8), np.uint8), mv.DeviceArray(n, np.uint32)
            measure("dilation_list", lambda: svo.dilation_cells_device(e, n, xyz, at, cnt))
        m = measure("erosion_count", lambda: svo.erosion_voxels_device(e))
        if m:
            vi = mv.DeviceArray(m, np.uint32)
            measure("erosion_list", lambda: svo.erosion_voxels_device(e, m, vi))
    elif op == "steps":
        measure("dilate1", lambda: svo.dilate(e, 1), before=restore)
        restore()
        svo.dilate(e, 1)
        grown = bk.snapshot(mv, svo)
        measure("erode1", lambda: svo.erode(e, 1), before=lambda: restore(grown), voxels_before=svo.info().numberOfVoxels)
        restore()
        n = svo.dilation_cells_device(e)
        xyz, at = mv.DeviceArray((n, 3), np.uint32), mv.DeviceArray((n, 8), np.uint8)

        def list_edit():
            svo.dilation_cells_device(e, n, xyz, at, None)
            svo.edit_voxels(xyz, at)
            return n

        measure("list_edit", list_edit, before=restore)
    elif op == "close":
        def sequence(k):
            added = sum(svo.dilate(e, 1) for _ in range(k))
            return added - sum(svo.erode(e, 1) for _ in range(k))

        for k in [int(v) for v in args.close_steps.split(",")]:
            results = set()
            try:  # alternating: both forms see the same machine
                (ms, one), (ms_steps, many) = bk.timed_each(mv, [lambda: svo.close(e, k), lambda: sequence(k)], args.reps, args.warmup, before=restore,
                                                            after=lambda j, result: results.add(result))
            except mv.MvrtError as err:
                bk.emit(base, op="close%d" % k, refused=str(err))
                break
            assert len(results) == 1, results  # the same net cells either way
            bk.emit(base, op="close%d" % k, ms=ms, all_ms=one, result=results.pop(), voxels_after=svo.info().numberOfVoxels)
            bk.emit(base, op="close%d_steps" % k, ms=ms_steps, all_ms=many, calls=2 * k)


def line(r):
    what = "%9.2f ms" % r["ms"] if "ms" in r else r.get("refused") or r.get("failed")
    return "%-7s %5s %-6s %-16s %10s voxels  %s  -> %s" % (r.get("scene", r.get("step")), r.get("grid", ""), r.get("element", ""), r.get("op", ""), r.get("voxels", ""), what,
                                                           r.get("result", ""))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=bk.parse_scenes, default="dragon,tunnel")
    ap.add_argument("--elements", default="faces,cube")
    ap.add_argument("--ops", default="listings,steps,close")
    ap.add_argument("--close-steps", default="1,2,4")
    bk.add_step_args(ap, reps=5, warmup=1, step_timeout=360)
    args = ap.parse_args()
    if args.step:
        return step(args)
    steps = ["%s:%d:%s:%s" % (name, res, op, e) for name, res in args.scenes for op in args.ops.split(",") for e in args.elements.split(",")]
    rows, rc = bk.run_steps(__file__, steps, lambda s: bk.flags(args, "reps", "warmup", "close_steps"), args.step_timeout, args.out)
    bk.print_table(rows, line)
    return rc


if __name__ == "__main__":
    sys.exit(main())
