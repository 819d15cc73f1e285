#!/usr/bin/env python3
"""usage: tools/ball_bench.py [--scenes dragon[:grid],tunnel[:grid]] [--radii 1,3,9,16,64] [--close-radius 16] [--cube-steps 4] [--reps 3] [--warmup 1] [--step-timeout 420]
                           [--out profiles/ball_bench.json]

Cost of the round offsets on the procedural stand-ins (dragon 2048^3, tunnel 4096^3), per scene:
  distance_count / distance_list   mvrt_svo_distance_cells at each radius2 of --radii, the sizing call and the listing into device arrays; with the seeds, the
                                   records of the passes along x, y and z, the cells of the band (mvrt_test_ball_stats) and the peak scratch of the call
                                   (mvrt_test_peak_bytes: the most the library held during the call minus what it held before)
  close_ball                       mvrt_svo_close_ball at --close-radius in ONE call, with the peak scratch
  close_cube                       mvrt_svo_close( CUBE, --cube-steps ) from the step morphology next to it: the yardstick.  ratio = close_ball / close_cube
The octree is rebuilt from its own voxel list before every timed in-place call, outside the clock; the two closings alternate inside one process, so that both
see the same machine.  Median of --reps calls after --warmup calls; host clock around each call (every call blocks).  A call the library refuses (a pass of
2^32 - 1 records or more) is reported with its message, never guessed.
Every step runs in a child process of its own under --step-timeout seconds; a step that fails, is killed or runs out of time ends the run: nothing more is
started on the GPU behind it."""
import argparse
import sys

import numpy as np

import benchkit as bk


def step(args):
    """one child process: prints one JSON row per measurement"""
    import massivevoxelraytracing_amd as mv
    mv.set_device(0)
    name, res, op = args.step.split(":")
    res = int(res)
    svo, origin, dps = bk.built(mv, name, res)
    base = dict(scene=name, grid=res, voxels=svo.info().numberOfVoxels)
    held = []

    def arm():  # the peak scratch of a call: the most the library held during it minus what it held before (host-side counters: no device work)
        held.append(mv.allocation_state()[1])
        mv.peak_bytes(reset=True)

    def peak():
        return mv.peak_bytes() - held[-1]

    def measured(label, fn, **kw):
        """-> the last result"""
        seen = {}
        try:
            ms, ts = bk.timed(mv, fn, args.reps, args.warmup, before=arm, after=lambda j, result: seen.update(result=result, peak_scratch_bytes=peak()))
        except mv.MvrtError as err:
            bk.emit(base, op=label, refused=str(err), **dict(kw, **mv.ball_stats()))
            return None
        bk.emit(base, op=label, ms=ms, all_ms=ts, **dict(kw, **mv.ball_stats()), **seen)
        return seen["result"]

    if op == "distance":
        for rho in [int(v) for v in args.radii.split(",")]:
            n = measured("distance_count", lambda: svo.distance_cells_device(rho), radius2=rho)
            if n:
                xyz, d2, near, at = mv.DeviceArray((n, 3), np.uint32), mv.DeviceArray(n, np.uint32), mv.DeviceArray(n, np.uint32), mv.DeviceArray((n, 8), np.uint8)
                measured("distance_list", lambda: svo.distance_cells_device(rho, n, xyz, d2, near, at), radius2=rho)
                del xyz, d2, near, at
    elif op == "close":
        as_built = bk.snapshot(mv, svo)
        rho, k = args.close_radius, args.cube_steps
        seen = [{}, {}]

        def restore():
            svo.build_voxels(as_built[0], as_built[1], origin=origin, dps=dps, gridRes=res)
            arm()

        try:  # alternating: both forms see the same machine
            (ball_ms, ball), (cube_ms, cube) = bk.timed_each(
                mv, [lambda: svo.close_ball(rho), lambda: svo.close(mv.MORPH_CUBE, k)], args.reps, args.warmup, before=restore,
                after=lambda j, result: seen[j].update(result=result, voxels_after=svo.info().numberOfVoxels, peak_scratch_bytes=peak()))
        except mv.MvrtError as err:
            bk.emit(base, op="close", refused=str(err), radius2=rho, cube_steps=k)
            return
        bk.emit(base, op="close_ball", ms=ball_ms, all_ms=ball, radius2=rho, **seen[0])
        bk.emit(base, op="close_cube", ms=cube_ms, all_ms=cube, cube_steps=k, **seen[1])
        bk.emit(base, op="close_ratio", ratio=float(ball_ms / cube_ms), radius2=rho, cube_steps=k)


def line(r):
    what = "%9.2f ms" % r["ms"] if "ms" in r else r.get("refused") or r.get("failed") or "ratio %.3f" % r.get("ratio", 0)
    return "%-7s %5s %-15s rho %-5s %10s voxels  %s  -> %s  records %s" % (r.get("scene", r.get("step")), r.get("grid", ""), r.get("op", ""), r.get("radius2", ""),
                                                                          r.get("voxels", ""), what, r.get("result", ""), r.get("records", ""))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=bk.parse_scenes, default="dragon,tunnel")
    ap.add_argument("--ops", default="distance,close")
    ap.add_argument("--radii", default="1,3,9,16,64")
    ap.add_argument("--close-radius", type=int, default=16)
    ap.add_argument("--cube-steps", type=int, default=4)
    bk.add_step_args(ap, reps=3, warmup=1, step_timeout=420)
    args = ap.parse_args()
    if args.step:
        return step(args)
    steps = ["%s:%d:%s" % (name, res, op) for name, res in args.scenes for op in args.ops.split(",")]
    rows, rc = bk.run_steps(__file__, steps, lambda s: bk.flags(args, "reps", "warmup", "radii", "close_radius", "cube_steps"), args.step_timeout, args.out)
    bk.print_table(rows, line)
    return rc


if __name__ == "__main__":
    sys.exit(main())
