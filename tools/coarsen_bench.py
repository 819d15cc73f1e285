#!/usr/bin/env python3
"""usage: tools/coarsen_bench.py [--scenes dragon[:grid],tunnel[:grid]] [--reps 10] [--warmup 2] [--step-timeout 500] [--out profiles/coarsen_bench.json]

Cost of the level of detail from the voxels themselves on the procedural stand-ins (dragon 2048^3, tunnel 4096^3), for levelsDown k = 1, 2, 3 and L - 1:
  count         mvrt_svo_coarse_voxels, the sizing call with minCount 1: heads + ranks, the count back on the host (no reduce: every cell is kept)
  count_min2    the sizing call with minCount 2: heads + ranks + the segmented reduce + the scan of the keep flags
  list          mvrt_svo_coarse_voxels with minCount 1 into device arrays allocated before the clock starts: heads + ranks + reduce + emit
  coarsen       mvrt_svo_coarsen with minCount 1 into a second handle: the same list + the levels of the voxel-list build + the derived tables
  build_voxels  the only route without this feature: mvrt_svo_build_voxels into a second handle on device arrays of the shifted coordinates and the attributes,
                prepared outside the clock.  (Its 32-bit sums overflow in cells of more than 8.4 M voxels: at k = L - 1 its colours are wrong; its time stands.)
  read_voxels   once per scene: mvrt_svo_read_voxels into device arrays, a plain streaming pass over the same 16 bytes per voxel
coarsen and build_voxels alternate call by call inside one loop.  Median of --reps calls after --warmup calls, with the smallest and the largest; host clock
around each call (every call blocks).  One child process per scene under --step-timeout seconds; a step that fails, is killed or runs out of time ends the run:
nothing more is started on the GPU behind it."""
import argparse
import sys

import numpy as np

import benchkit as bk


def step(args):
    """one child process: prints one JSON row per measurement"""
    import massivevoxelraytracing_amd as mv
    mv.set_device(0)
    name, res = args.step.split(":")
    res = int(res)
    svo, origin, dps = bk.built(mv, name, res)
    n = svo.info().numberOfVoxels
    levels = svo.info().levels
    base = dict(scene=name, grid=res, voxels=n)

    def emit(**kw):
        if "all_ms" in kw:
            kw.update(min_ms=min(kw["all_ms"]), max_ms=max(kw["all_ms"]))
        bk.emit(base, **kw)

    def clock(*fns):
        return bk.timed_each(mv, fns, args.reps, args.warmup)

    xyz, attrs = mv.DeviceArray((n, 3), np.uint32), mv.DeviceArray((n, 8), np.uint8)
    (ms, ts), = clock(lambda: mv._check(mv.lib().mvrt_svo_read_voxels(svo._h, xyz.ptr, attrs.ptr, None)))
    emit(op="read_voxels", ms=ms, all_ms=ts, gb_per_s=n * 36 / (ms * 1e6))  # 16 B read, 20 B written per voxel
    fine = xyz.to_host()
    for k in sorted({1, 2, 3, levels - 1}):
        cells = svo.coarse_voxels_device(k)
        (ms, ts), (ms2, ts2) = clock(lambda: svo.coarse_voxels_device(k), lambda: svo.coarse_voxels_device(k, 2))
        emit(op="count", k=k, cells=cells, ms=ms, all_ms=ts)
        emit(op="count_min2", k=k, cells=svo.coarse_voxels_device(k, 2), ms=ms2, all_ms=ts2)
        cx, ca, cc = mv.DeviceArray((cells, 3), np.uint32), mv.DeviceArray((cells, 8), np.uint8), mv.DeviceArray(cells, np.uint32)
        (ms, ts), = clock(lambda: svo.coarse_voxels_device(k, 1, cells, cx, ca, cc))
        emit(op="list", k=k, cells=cells, ms=ms, all_ms=ts, voxels_per_s=n / (ms * 1e-3))
        del cx, ca, cc
        shifted = mv.DeviceArray.from_host(fine >> np.uint32(k))  # the parent's input, prepared outside the clock
        a, b = mv.IntersectorOctreeGPU(), mv.IntersectorOctreeGPU()
        coarse_dps = np.float32(np.float32(dps) * np.float32(2 ** k))
        (ms, ts), (msp, tsp) = clock(lambda: svo.coarsen(k, 1, 0, a), lambda: b.build_voxels(shifted, attrs, origin=origin, dps=coarse_dps, gridRes=res >> k))
        same = a.info().numberOfVoxels == b.info().numberOfVoxels == cells and a.info().numberOfNodes == b.info().numberOfNodes
        emit(op="coarsen", k=k, cells=cells, ms=ms, all_ms=ts, voxels_per_s=n / (ms * 1e-3))
        emit(op="build_voxels", k=k, cells=cells, ms=msp, all_ms=tsp, same_counts=bool(same), coarsen_speedup=msp / ms)
        del a, b, shifted


def line(r):
    what = "%9.2f ms  [%8.2f, %8.2f]" % (r["ms"], r["min_ms"], r["max_ms"]) if "ms" in r else r.get("failed")
    return "%-7s %5s %-13s k %3s %10s voxels %10s cells  %s" % (r.get("scene", r.get("step")), r.get("grid", ""), r.get("op", ""), r.get("k", ""), r.get("voxels", ""),
                                                               r.get("cells", ""), what)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=bk.parse_scenes, default="dragon,tunnel")
    bk.add_step_args(ap, reps=10, warmup=2, step_timeout=500)
    args = ap.parse_args()
    if args.step:
        return step(args)
    rows, rc = bk.run_steps(__file__, ["%s:%d" % scene for scene in args.scenes], lambda s: bk.flags(args, "reps", "warmup"), args.step_timeout, args.out)
    bk.print_table(rows, line)
    return rc


if __name__ == "__main__":
    sys.exit(main())
