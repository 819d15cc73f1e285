#!/usr/bin/env python3
"""usage: tools/ball_bench.py [--scenes dragon,tunnel] [--radii 1,3,9,16,64] [--close-radius 16] [--cube-steps 4] [--reps 3] [--warmup 1] [--step-timeout 420]
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
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRID = {"dragon": 2048, "tunnel": 4096}


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
        print(json.dumps(dict(kw, **base)), flush=True)

    def clocked(fn):
        """-> (ms, result, peak scratch bytes)"""
        mv.synchronize()
        held = mv.allocation_state()[1]
        mv.peak_bytes(reset=True)
        t0 = time.perf_counter()
        result = fn()
        ms = (time.perf_counter() - t0) * 1e3
        return ms, result, mv.peak_bytes() - held

    def timed(label, fn, **kw):
        ts, result, peak = [], None, 0
        for i in range(args.warmup + args.reps):
            try:
                ms, result, peak = clocked(fn)
            except mv.MvrtError as err:
                emit(op=label, refused=str(err), **dict(kw, **mv.ball_stats()))
                return None
            if i >= args.warmup:
                ts.append(ms)
        emit(op=label, ms=float(np.median(ts)), all_ms=ts, result=result, peak_scratch_bytes=peak, **dict(kw, **mv.ball_stats()))
        return result

    if op == "distance":
        for rho in [int(v) for v in args.radii.split(",")]:
            n = timed("distance_count", lambda: svo.distance_cells_device(rho), radius2=rho)
            if n:
                xyz, d2, near, at = mv.DeviceArray((n, 3), np.uint32), mv.DeviceArray(n, np.uint32), mv.DeviceArray(n, np.uint32), mv.DeviceArray((n, 8), np.uint8)
                timed("distance_list", lambda: svo.distance_cells_device(rho, n, xyz, d2, near, at), radius2=rho)
                del xyz, d2, near, at
    elif op == "close":
        as_built = snapshot(mv, svo)
        rho, k = args.close_radius, args.cube_steps
        ball, cube, results, peaks = [], [], {}, {}
        try:
            for i in range(args.warmup + args.reps):  # alternating: both forms see the same machine
                for label, ts, fn in (("close_ball", ball, lambda: svo.close_ball(rho)), ("close_cube", cube, lambda: svo.close(mv.MORPH_CUBE, k))):
                    svo.build_voxels(as_built[0], as_built[1], origin=origin, dps=dps, gridRes=res)
                    ms, results[label], peaks[label] = clocked(fn)
                    results[label + "_after"] = svo.info().numberOfVoxels
                    if i >= args.warmup:
                        ts.append(ms)
        except mv.MvrtError as err:
            emit(op="close", refused=str(err), radius2=rho, cube_steps=k)
            return
        emit(op="close_ball", ms=float(np.median(ball)), all_ms=ball, result=results["close_ball"], voxels_after=results["close_ball_after"], radius2=rho,
             peak_scratch_bytes=peaks["close_ball"])
        emit(op="close_cube", ms=float(np.median(cube)), all_ms=cube, result=results["close_cube"], voxels_after=results["close_cube_after"], cube_steps=k,
             peak_scratch_bytes=peaks["close_cube"])
        emit(op="close_ratio", ratio=float(np.median(ball) / np.median(cube)), radius2=rho, cube_steps=k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="dragon,tunnel")
    ap.add_argument("--ops", default="distance,close")
    ap.add_argument("--radii", default="1,3,9,16,64")
    ap.add_argument("--close-radius", type=int, default=16)
    ap.add_argument("--cube-steps", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--step-timeout", type=int, default=420)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        return step(args)
    steps = [":".join((s, op)) for s in args.scenes.split(",") for op in args.ops.split(",")]
    rows, rc = [], 0
    for s in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", s, "--reps", str(args.reps), "--warmup", str(args.warmup), "--radii", args.radii,
               "--close-radius", str(args.close_radius), "--cube-steps", str(args.cube_steps)]
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
        what = "%9.2f ms" % r["ms"] if "ms" in r else r.get("refused") or r.get("failed") or "ratio %.3f" % r.get("ratio", 0)
        print("%-7s %5s %-15s rho %-5s %10s voxels  %s  -> %s  records %s" % (r.get("scene", r.get("step")), r.get("grid", ""), r.get("op", ""), r.get("radius2", ""),
                                                                          r.get("voxels", ""), what, r.get("result", ""), r.get("records", "")), file=sys.stderr)
    return rc


if __name__ == "__main__":
    sys.exit(main())
