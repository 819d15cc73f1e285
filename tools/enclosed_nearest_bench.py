#!/usr/bin/env python3
"""usage: tools/enclosed_nearest_bench.py [--scenes dragon:2048,tunnel:4096,dragon:1024] [--reps 5] [--warmup 1] [--step-timeout 420]
                                         [--out profiles/enclosed_nearest_bench.json]

Cost of the nearest voxel of every enclosed cell (mvrt_svo_enclosed_nearest / mvrt_svo_fill_enclosed_nearest) next to the calls that give the
same cells without it, on the procedural stand-ins:
  size          the sizing calls of mvrt_svo_enclosed_nearest and mvrt_svo_enclosed_cells: the classification alone, no pass
  list          mvrt_svo_enclosed_nearest into device arrays next to mvrt_svo_enclosed_cells into device arrays (the yardstick)
  fill          mvrt_svo_fill_enclosed_nearest next to mvrt_svo_fill_enclosed (the yardstick), each on the octree as built: rebuilt from its own voxel list
                before every timed call, outside the clock
Every call is reported (all_ms), with its median; host clock around each call (every call blocks until its counts are back); output arrays are allocated before
the clock starts.  Per new call also the peak scratch (mvrt_test_peak_bytes around one call) and the figures of mvrt_test_enclosed_nearest_stats: gaps and
longest gap per axis, deepest d2.  A call the library refuses, or whose scratch does not fit the device, is reported with the library's message, never guessed.
Every step runs in a child process of its own under `timeout -k 10 --step-timeout`; a step that fails, is killed or runs out of time ends the run: nothing more
is started on the GPU behind it.  A child sizes no thread pool of its own."""
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
    n_vox = svo.info().numberOfVoxels
    n_cells, n_regions = svo.enclosed_cells_device()
    base = dict(scene=name, grid=res, voxels=n_vox, nCells=n_cells, nRegions=n_regions)

    def measure(label, fn, before=None, stats=False):
        try:
            peak = bk.peak_of(mv, (lambda: (before(), fn())) if before else fn)  # (with `before` the peak covers the rebuild too: reported as such)
            ms, ts = bk.timed(mv, fn, args.reps, args.warmup, before=before)
        except mv.MvrtError as e:
            bk.emit(base, op=label, refused=str(e), peak_bytes=mv.peak_bytes() - mv.allocation_state()[1])
            return None
        bk.emit(base, op=label, ms=ms, all_ms=ts, peak_bytes=peak, peak_includes_rebuild=bool(before), **(mv.enclosed_nearest_stats() if stats else {}))
        return ms

    if op == "size":
        a = measure("nearest_size", svo.enclosed_nearest_device)
        b = measure("cells_size", svo.enclosed_cells_device)
        bk.emit(base, op="size_ratio", ratio=a / b)
    elif op == "list":
        if n_cells == 0 or n_cells >= 1 << 32:
            bk.emit(base, op="nearest_list", skipped="%d cells" % n_cells)
            return
        xyz, region = mv.DeviceArray((n_cells, 3), np.uint32), mv.DeviceArray(n_cells, np.uint32)
        d2, near, at = mv.DeviceArray(n_cells, np.uint32), mv.DeviceArray(n_cells, np.uint32), mv.DeviceArray((n_cells, 8), np.uint8)
        a = measure("nearest_list", lambda: svo.enclosed_nearest_device(n_cells, xyz, region, d2, near, at), stats=True)
        b = measure("cells_list", lambda: svo.enclosed_cells_device(n_cells, xyz, region))
        if a and b:
            bk.emit(base, op="list_ratio", ratio=a / b, cells_per_s=n_cells / (a * 1e-3))
    elif op == "fill":
        if n_cells == 0 or n_cells + n_vox >= (1 << 32) - 1:
            bk.emit(base, op="nearest_fill", skipped="%d cells" % n_cells)
            return
        xyz, attrs = bk.snapshot(mv, svo)
        rebuild = lambda: svo.build_voxels(xyz, attrs, origin=origin, dps=dps, gridRes=res)
        filled = []
        a = measure("nearest_fill", lambda: filled.append(svo.fill_enclosed_nearest()), before=rebuild, stats=True)
        b = measure("plain_fill", lambda: filled.append(svo.fill_enclosed()), before=rebuild)
        assert set(filled) <= {n_cells}, (set(filled), n_cells)
        if a and b:
            bk.emit(base, op="fill_ratio", ratio=a / b, voxels_after=svo.info().numberOfVoxels, cells_left=svo.enclosed_cells_device()[0])


def line(r):
    what = "%9.2f ms" % r["ms"] if "ms" in r else "x %.2f" % r["ratio"] if "ratio" in r else r.get("refused") or r.get("skipped") or r.get("failed")
    return "%-7s %5s %-13s %10s voxels %11s cells %5s regions  %s" % (r.get("scene", r.get("step")), r.get("grid", ""), r.get("op", ""), r.get("voxels", ""), r.get("nCells", ""),
                                                                      r.get("nRegions", ""), what)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=bk.parse_scenes, default="dragon:2048,tunnel:4096,dragon:1024")
    ap.add_argument("--ops", default="size,list,fill")
    bk.add_step_args(ap, reps=5, warmup=1, step_timeout=420)
    args = ap.parse_args()
    if args.step:
        return step(args)
    steps = ["%s:%d:%s" % (name, res, op) for name, res in args.scenes for op in args.ops.split(",")]
    rows, rc = bk.run_steps(__file__, steps, lambda s: bk.flags(args, "reps", "warmup"), args.step_timeout, args.out)
    bk.print_table(rows, line)
    return rc


if __name__ == "__main__":
    sys.exit(main())
