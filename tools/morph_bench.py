#!/usr/bin/env python3
"""usage: tools/morph_bench.py [--scenes dragon,tunnel] [--reps 5] [--warmup 1] [--step-timeout 360] [--close-steps 1,2,4] [--out profiles/morph_bench.json]

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
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRID = {"dragon": 2048, "tunnel": 4096}
ELEMENT = {"faces": 0, "cube": 1}


def built(mv, name, res):
    from massivevoxelraytracing_amd import scenes
    verts, cols, emis = scenes.SCENES[name](1.0)
    origin, dps = scenes.bounding_grid(verts, res)
    svo = mv.IntersectorOctreeGPU()
    svo.build(verts, cols, emis, None, origin, dps, res)
    return svo, origin, dps


def snapshot(mv, svo):
    n = svo.info().numberOfVoxels
    xyz, attrs = mv.DeviceArray((n, 3), np.uint32), mv.DeviceArray((n, 8), np.uint8)
    mv._check(mv.lib().mvrt_svo_read_voxels(svo._h, xyz.ptr, attrs.ptr, None))
    return xyz, attrs


def step(args):
    """one child process: prints one JSON row per measurement"""
    import massivevoxelraytracing_amd as mv
    mv.set_device(0)
    name, op, ename = args.step.split(":")
    e, res = ELEMENT[ename], GRID[name]
    svo, origin, dps = built(mv, name, res)
    n_vox = svo.info().numberOfVoxels
    base = dict(scene=name, grid=res, voxels=n_vox, element=ename)
    as_built = snapshot(mv, svo)

    def restore(list_=as_built):
        svo.build_voxels(list_[0], list_[1], origin=origin, dps=dps, gridRes=res)

    def emit(**kw):
        print(json.dumps(dict(kw, **base)), flush=True)

    def timed(label, fn, before=None, **kw):
        ts, result = [], None
        for i in range(args.warmup + args.reps):
            if before:
                before()
            mv.synchronize()
            t0 = time.perf_counter()
            try:
                result = fn()
            except mv.MvrtError as err:
                emit(op=label, refused=str(err), **kw)
                return None
            if i >= args.warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
        emit(op=label, ms=float(np.median(ts)), all_ms=ts, result=result, **kw)
        return result

    if op == "listings":
        n = timed("dilation_count", lambda: svo.dilation_cells_device(e))
        if n:
            xyz, at, cnt = mv.DeviceArray((n, 3), np.uint32), mv.DeviceArray((n, 8), np.uint8), mv.DeviceArray(n, np.uint32)
            timed("dilation_list", lambda: svo.dilation_cells_device(e, n, xyz, at, cnt))
        m = timed("erosion_count", lambda: svo.erosion_voxels_device(e))
        if m:
            vi = mv.DeviceArray(m, np.uint32)
            timed("erosion_list", lambda: svo.erosion_voxels_device(e, m, vi))
    elif op == "steps":
        timed("dilate1", lambda: svo.dilate(e, 1), before=restore)
        restore()
        svo.dilate(e, 1)
        grown = snapshot(mv, svo)
        timed("erode1", lambda: svo.erode(e, 1), before=lambda: restore(grown), voxels_before=svo.info().numberOfVoxels)
        restore()
        n = svo.dilation_cells_device(e)
        xyz, at = mv.DeviceArray((n, 3), np.uint32), mv.DeviceArray((n, 8), np.uint8)

        def list_edit():
            svo.dilation_cells_device(e, n, xyz, at, None)
            svo.edit_voxels(xyz, at)
            return n

        timed("list_edit", list_edit, before=restore)
    elif op == "close":
        def sequence(k):
            added = sum(svo.dilate(e, 1) for _ in range(k))
            return added - sum(svo.erode(e, 1) for _ in range(k))

        for k in [int(v) for v in args.close_steps.split(",")]:
            one, many, results = [], [], set()
            try:
                for i in range(args.warmup + args.reps):  # alternating: both forms see the same machine
                    for ts, fn in ((one, lambda: svo.close(e, k)), (many, lambda: sequence(k))):
                        restore()
                        mv.synchronize()
                        t0 = time.perf_counter()
                        results.add(fn())
                        if i >= args.warmup:
                            ts.append((time.perf_counter() - t0) * 1e3)
            except mv.MvrtError as err:
                emit(op="close%d" % k, refused=str(err))
                break
            assert len(results) == 1, results  # the same net cells either way
            emit(op="close%d" % k, ms=float(np.median(one)), all_ms=one, result=results.pop(), voxels_after=svo.info().numberOfVoxels)
            emit(op="close%d_steps" % k, ms=float(np.median(many)), all_ms=many, calls=2 * k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="dragon,tunnel")
    ap.add_argument("--elements", default="faces,cube")
    ap.add_argument("--ops", default="listings,steps,close")
    ap.add_argument("--close-steps", default="1,2,4")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--step-timeout", type=int, default=360)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        return step(args)
    steps = [":".join((s, op, e)) for s in args.scenes.split(",") for op in args.ops.split(",") for e in args.elements.split(",")]
    rows, rc = [], 0
    for s in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", s, "--reps", str(args.reps), "--warmup", str(args.warmup), "--close-steps", args.close_steps]
        print("step", s, flush=True)
        try:
            out = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            rows.append(dict(step=s, failed="no result within %d s" % args.step_timeout))
            rc = 1
            break
        for line in out.stdout.decode().splitlines():
            if line.startswith("{"):
                rows.append(json.loads(line))
                print(line, flush=True)
        if out.returncode != 0:
            rows.append(dict(step=s, failed="exit status %d" % out.returncode))
            rc = 1
            break  # nothing more is started on the GPU behind a step that failed
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
    for r in rows:
        what = "%9.2f ms" % r["ms"] if "ms" in r else r.get("refused") or r.get("failed")
        print("%-7s %5s %-6s %-16s %10s voxels  %s  -> %s" % (r.get("scene", r.get("step")), r.get("grid", ""), r.get("element", ""), r.get("op", ""), r.get("voxels", ""), what,
                                                             r.get("result", "")), file=sys.stderr)
    return rc


if __name__ == "__main__":
    sys.exit(main())
