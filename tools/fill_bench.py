#!/usr/bin/env python3
"""usage: tools/fill_bench.py [--scenes dragon[:grid],tunnel[:grid]] [--reps 10] [--warmup 2] [--step-timeout 360] [--out profiles/fill_bench.json] [--no-host-method]

Cost of classifying and filling the enclosed empty cells on the procedural stand-ins (dragon 2048^3, tunnel 4096^3):
  count   mvrt_svo_enclosed_cells, the sizing call: linear keys + radix sort + unions + flatten + scan, counts back on the host
  list    mvrt_svo_enclosed_cells into device arrays: the same + emit + radix sort of (code, root) + ranks
  fill    mvrt_svo_fill_enclosed on the octree as built (rebuilt from its own voxel list before every call, outside the clock)
Median of --reps calls after --warmup calls; host clock around each call (every call blocks until its counts are back).  Output arrays are allocated before the
clock starts.  A count beyond what one listing or one octree holds, or beyond --max-cells (device memory: a listing keeps about 60 B per cell in flight), is
reported with the library's message or as skipped, never guessed.
Every step runs in a child process of its own under --step-timeout seconds; a step that fails, is killed or runs out of time ends the run: nothing more is
started on the GPU behind it.
Once, on the dragon at --host-grid (default 1024, the largest power of two whose dense int32 label array, 4 B per cell, stays within 4 GiB of host memory): the
only route without this feature -- mvrt_svo_read_voxels + a dense host flood fill (scipy.ndimage.label where scipy is installed, else the numpy propagation
of tests/fill_expected.py), next to the GPU's time for the same grid."""
import argparse
import os
import sys
import time

import numpy as np

import benchkit as bk


def host_flood_fill(xyz, res):
    """-> (number of enclosed cells, number of regions, method)"""
    solid = np.zeros((res,) * 3, bool)
    solid[xyz[:, 0], xyz[:, 1], xyz[:, 2]] = True
    try:
        from scipy import ndimage
    except ImportError:
        sys.path.insert(0, os.path.join(bk.ROOT, "tests"))
        import fill_expected as F
        want = F.enclosed(xyz, res)
        return len(want["xyz"]), want["nRegions"], "numpy propagation"
    label, _ = ndimage.label(~solid)
    outside = np.zeros(int(label.max()) + 1, bool)
    for axis in range(3):
        for side in (0, res - 1):
            s = [slice(None)] * 3
            s[axis] = side
            outside[np.unique(label[tuple(s)])] = True
    outside[0] = True  # label 0 = the voxels
    counts = np.bincount(label.reshape(-1), minlength=len(outside))
    return int(counts[~outside].sum()), int((~outside).sum()), "scipy.ndimage.label"


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

    if op == "cells":
        ms, ts = bk.timed(mv, svo.enclosed_cells_device, args.reps, args.warmup)
        bk.emit(base, op="count", ms=ms, all_ms=ts)
        if n_cells == 0 or n_cells > args.max_cells:
            if n_cells >= 1 << 32:
                try:
                    svo.enclosed_cells_device(n_cells, mv.DeviceArray(3, np.uint32), None)  # refused on the host, before anything is written
                except mv.MvrtError as e:
                    bk.emit(base, op="list", refused=str(e))
                    return
            bk.emit(base, op="list", skipped="no cells" if n_cells == 0 else "%d cells exceed --max-cells %d" % (n_cells, args.max_cells))
            return
        xyz, region = mv.DeviceArray((n_cells, 3), np.uint32), mv.DeviceArray(n_cells, np.uint32)
        ms, ts = bk.timed(mv, lambda: svo.enclosed_cells_device(n_cells, xyz, region), args.reps, args.warmup)
        bk.emit(base, op="list", ms=ms, all_ms=ts, cells_per_s=n_cells / (ms * 1e-3))
    elif op == "fill":
        if n_cells == 0 or n_cells > args.max_cells:
            if n_cells + n_vox >= (1 << 32) - 1:
                try:
                    svo.fill_enclosed()
                except mv.MvrtError as e:
                    bk.emit(base, op="fill", refused=str(e))
                    return
            bk.emit(base, op="fill", skipped="no cells" if n_cells == 0 else "%d cells exceed --max-cells %d" % (n_cells, args.max_cells))
            return
        xyz, attrs = bk.snapshot(mv, svo)
        filled = []
        ms, ts = bk.timed(mv, lambda: filled.append(svo.fill_enclosed()), args.reps, args.warmup,
                       before=lambda: svo.build_voxels(xyz, attrs, origin=origin, dps=dps, gridRes=res))
        assert set(filled) == {n_cells}, (set(filled), n_cells)
        bk.emit(base, op="fill", ms=ms, all_ms=ts, voxels_after=svo.info().numberOfVoxels, cells_left=svo.enclosed_cells_device()[0])
    elif op == "host":
        ms, ts = bk.timed(mv, svo.enclosed_cells_device, args.reps, args.warmup)
        bk.emit(base, op="count", ms=ms, all_ms=ts)
        t0 = time.perf_counter()
        xyz, _ = svo.read_voxels()
        cells, regions, method = host_flood_fill(xyz, res)
        bk.emit(base, op="host_flood_fill", ms=(time.perf_counter() - t0) * 1e3, method=method, host_cells=cells, host_regions=regions,
             equal_to_gpu=bool((cells, regions) == (n_cells, n_regions)))


def line(r):
    what = "%9.2f ms" % r["ms"] if "ms" in r else r.get("refused") or r.get("skipped") or r.get("failed")
    return "%-7s %5s %-16s %10s voxels %11s cells %7s regions  %s" % (r.get("scene", r.get("step")), r.get("grid", ""), r.get("op", ""), r.get("voxels", ""), r.get("nCells", ""),
                                                                      r.get("nRegions", ""), what)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=bk.parse_scenes, default="dragon,tunnel")
    ap.add_argument("--max-cells", type=int, default=1 << 30)
    ap.add_argument("--host-grid", type=int, default=1024)
    ap.add_argument("--no-host-method", action="store_true")
    bk.add_step_args(ap, reps=10, warmup=2, step_timeout=360)
    args = ap.parse_args()
    if args.step:
        return step(args)
    steps = ["%s:%d:%s" % (name, res, op) for name, res in args.scenes for op in ("cells", "fill")]
    if "dragon" in [name for name, _ in args.scenes] and not args.no_host_method:
        steps.append("dragon:%d:host" % args.host_grid)
    rows, rc = bk.run_steps(__file__, steps, lambda s: bk.flags(args, "reps", "warmup", "max_cells"), args.step_timeout, args.out)
    bk.print_table(rows, line)
    return rc


if __name__ == "__main__":
    sys.exit(main())
