#!/usr/bin/env python3
"""usage: tools/components_bench.py [--scenes dragon[:grid],tunnel[:grid]] [--reps 5] [--warmup 1] [--step-timeout 360] [--out profiles/components_bench.json]

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
import sys

import numpy as np

import benchkit as bk

ELEMENT = {"faces": 0, "cube": 1}


def step(args):
    """one child process: prints one JSON row per measurement"""
    import massivevoxelraytracing_amd as mv
    mv.set_device(0)
    name, res, op = args.step.split(":")
    res = int(res)
    svo, origin, dps = bk.built(mv, name, res)
    base = dict(scene=name, grid=res, voxels=svo.info().numberOfVoxels)

    def measure(label, fn, before=None, **kw):
        return bk.timed_or_refused(mv, base, label, fn, args.reps, args.warmup, before, **kw)

    if op == "listings":
        for ename, e in ELEMENT.items():
            got = measure("components_count", lambda: svo.components_device(e), element=ename)
            if got:
                n = got[0]
                label, size = mv.DeviceArray(base["voxels"], np.uint32), mv.DeviceArray(n, np.uint32)
                first, box = mv.DeviceArray(n, np.uint32), mv.DeviceArray((n, 6), np.uint32)
                measure("components_list", lambda: svo.components_device(e, label, n, size, first, box), element=ename)
        measure("erosion_count", lambda: svo.erosion_voxels_device(ELEMENT["cube"]), element="cube")
        measure("enclosed_count", lambda: svo.enclosed_cells_device())
    elif op == "keep":
        e = ELEMENT["cube"]
        debris = np.random.default_rng(5).integers(0, res, (args.debris, 3)).astype(np.uint32)
        svo.edit_voxels(debris, np.full((len(debris), 8), 255, np.uint8))
        base["voxels"] = svo.info().numberOfVoxels
        with_debris = bk.snapshot(mv, svo)

        def restore():
            svo.build_voxels(with_debris[0], with_debris[1], origin=origin, dps=dps, gridRes=res)

        measure("keep_largest1", lambda: svo.keep_components(e, 1, 1), before=restore, element="cube")

        def list_edit():
            n, _ = svo.components_device(e)
            label, size = mv.DeviceArray(base["voxels"], np.uint32), mv.DeviceArray(n, np.uint32)
            svo.components_device(e, label, n, size)
            gone = label.to_host() != np.argmax(size.to_host())  # (argmax: the first of the largest)
            xyz = with_debris[0].to_host()[gone]
            svo.edit_voxels(xyz, None, np.zeros(len(xyz), np.uint8))
            return [int(gone.sum()), 1]

        measure("list_edit", list_edit, before=restore, element="cube")


def line(r):
    what = "%9.2f ms" % r["ms"] if "ms" in r else r.get("refused") or r.get("failed")
    return "%-7s %5s %-6s %-16s %10s voxels  %s  -> %s" % (r.get("scene", r.get("step")), r.get("grid", ""), r.get("element", ""), r.get("op", ""), r.get("voxels", ""), what,
                                                           r.get("result", ""))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=bk.parse_scenes, default="dragon,tunnel")
    ap.add_argument("--ops", default="listings,keep")
    ap.add_argument("--debris", type=int, default=100000)
    bk.add_step_args(ap, reps=5, warmup=1, step_timeout=360)
    args = ap.parse_args()
    if args.step:
        return step(args)
    steps = ["%s:%d:%s" % (name, res, op) for name, res in args.scenes for op in args.ops.split(",")]
    rows, rc = bk.run_steps(__file__, steps, lambda s: bk.flags(args, "reps", "warmup", "debris"), args.step_timeout, args.out)
    bk.print_table(rows, line)
    return rc


if __name__ == "__main__":
    sys.exit(main())
