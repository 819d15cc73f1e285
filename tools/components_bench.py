#!/usr/bin/env python3
"""usage: tools/components_bench.py [--scenes dragon,tunnel] [--reps 5] [--warmup 1] [--step-timeout 360] [--out profiles/components_bench.json]

Cost of the component calls on the procedural stand-ins (dragon 2048^3, tunnel 4096^3), per scene:
  components_count / components_list   mvrt_svo_components with faces and with cube: the sizing call, and the listing of all four arrays into device arrays
  erosion_count (cube)                 mvrt_svo_erosion_voxels, the sizing call: 26 presence searches per voxel against the 13 of the cube's half here
  enclosed_count                       mvrt_svo_enclosed_cells, the sizing call: the same union-find, over the gaps of the empty cells
  keep_largest1                        mvrt_svo_keep_components( cube, 1, 1 ) on the octree as built plus a sprinkle of debris voxels
  list_edit                            the same removal by hand: the labels and sizes to the host, the voxels of every component but the first largest
                                       back through mvrt_svo_edit_voxels with MVRT_VOXEL_REMOVE
The debris (--debris voxels at seeded random cells, set with mvrt_svo_edit_voxels before the clock starts) gives the selection something to drop: the scenes
themselves may well be one component.  The octree is rebuilt from its voxel list before every timed in-place call, outside the clock.  Median of --reps calls
after --warmup calls; host clock around each call (every call blocks).  A call the library refuses is reported with its message, never guessed.
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
    name, op = args.step.split(":")
    res = GRID[name]
    svo, origin, dps = built(mv, name, res)
    base = dict(scene=name, grid=res, voxels=svo.info().numberOfVoxels)

    def emit(**kw):
        print(json.dumps(dict(base, **kw)), flush=True)

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
        for ename, e in ELEMENT.items():
            got = timed("components_count", lambda: svo.components_device(e), element=ename)
            if got:
                n = got[0]
                label, size = mv.DeviceArray(base["voxels"], np.uint32), mv.DeviceArray(n, np.uint32)
                first, box = mv.DeviceArray(n, np.uint32), mv.DeviceArray((n, 6), np.uint32)
                timed("components_list", lambda: svo.components_device(e, label, n, size, first, box), element=ename)
        timed("erosion_count", lambda: svo.erosion_voxels_device(ELEMENT["cube"]), element="cube")
        timed("enclosed_count", lambda: svo.enclosed_cells_device())
    elif op == "keep":
        e = ELEMENT["cube"]
        debris = np.random.default_rng(5).integers(0, res, (args.debris, 3)).astype(np.uint32)
        svo.edit_voxels(debris, np.full((len(debris), 8), 255, np.uint8))
        base["voxels"] = svo.info().numberOfVoxels
        with_debris = snapshot(mv, svo)

        def restore():
            svo.build_voxels(with_debris[0], with_debris[1], origin=origin, dps=dps, gridRes=res)

        timed("keep_largest1", lambda: svo.keep_components(e, 1, 1), before=restore, element="cube")

        def list_edit():
            n, _ = svo.components_device(e)
            label, size = mv.DeviceArray(base["voxels"], np.uint32), mv.DeviceArray(n, np.uint32)
            svo.components_device(e, label, n, size)
            gone = label.to_host() != np.argmax(size.to_host())  # (argmax: the first of the largest)
            xyz = with_debris[0].to_host()[gone]
            svo.edit_voxels(xyz, None, np.zeros(len(xyz), np.uint8))
            return [int(gone.sum()), 1]

        timed("list_edit", list_edit, before=restore, element="cube")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="dragon,tunnel")
    ap.add_argument("--ops", default="listings,keep")
    ap.add_argument("--debris", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--step-timeout", type=int, default=360)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        return step(args)
    steps = [":".join((s, op)) for s in args.scenes.split(",") for op in args.ops.split(",")]
    rows, rc = [], 0
    for s in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", s, "--reps", str(args.reps), "--warmup", str(args.warmup), "--debris", str(args.debris)]
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
