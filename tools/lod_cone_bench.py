#!/usr/bin/env python3
"""usage: tools/lod_cone_bench.py [--reps 5] [--warmup 1] [--out profiles/lod_cone_bench.json] [--grids 2048,8192] [--steps pyramid,yardstick,cone,render]
                                  [--step-timeout 240]

Cone-limited rays on the dragon stand-in at 2048^3 and 8192^3: a 1920x1080 primary cast (the camera of bench.py, rays through the pixel centres).  Every step
of every grid runs in a child process of its own under `timeout` and builds the octree for itself; the first step that fails ends the run (nothing more is
started on the GPU) and what was measured up to there is still written.  Per grid:
  pyramid        the time of mvrt_svo_lod_prepare and mvrt_svo_lod_bytes beside the octree's own size
  yardstick      mvrt_trace_batch_range with tMax = +inf: the same per-lane kernel without a cone
  cone           mvrt_trace_batch_cone with coneA = 0 and coneB = lodScale * 2 tanHthetaY / H for lodScale 0, 0.5, 1, 2: ms per frame, descents per ray, the
                 histogram of the levels the rays stopped at; against one untimed yardstick call: never more descents on any ray, and at lodScale 0 the same t
  render         mvrt_render_primary (the streaming kernel) and mvrt_render_primary_lod at the same scales, voxel colours
Median of --reps calls after --warmup calls (mvrt_svo_lod_prepare included), host clock between device synchronisations."""
import argparse
import os
import sys
import time

import numpy as np

import benchkit as bk

W, H = 1920, 1080
SCALES = (0.0, 0.5, 1.0, 2.0)
STEPS = ("pyramid", "yardstick", "cone", "render")
MAXF = np.float32(3.402823466e38)
f32 = np.float32


def pixel_rays(cam):
    """CameraPinhole::shoot through the pixel centres, the operations of include/mvrt/device.hpp in fp32"""
    o, front, up, right, tan_h = cam[0:3], cam[3:6], cam[6:9], cam[9:12], f32(cam[12])
    x, y = np.meshgrid(np.arange(W, dtype=f32), np.arange(H, dtype=f32))
    xf, yf = ((x + f32(0.5)) / f32(W)).reshape(-1), ((y + f32(0.5)) / f32(H)).reshape(-1)
    a = (-tan_h + (tan_h - -tan_h) * xf).astype(f32)
    b = (tan_h + (-tan_h - tan_h) * yf).astype(f32)
    rd = (right[None, :] * (a * f32(W) / f32(H))[:, None] + up[None, :] * b[:, None] + front[None, :]).astype(f32)
    return np.ascontiguousarray(np.broadcast_to(o.astype(f32), rd.shape)), rd


def build_dragon(mv, res):
    """-> (octree, camera of bench.py, the fields every row carries, build time in ms)"""
    from massivevoxelraytracing_amd import scenes
    verts, cols, emis = scenes.SCENES["dragon"](1.0)
    origin, dps = scenes.bounding_grid(verts, res)
    svo = mv.IntersectorOctreeGPU()
    t0 = time.perf_counter()
    svo.build(verts, cols, emis, None, origin, dps, res)
    mv.synchronize()
    build_ms = (time.perf_counter() - t0) * 1e3
    info = svo.info()
    lo, hi = np.array(info.lower[:]), np.array(info.upper[:])
    centre = (lo + hi) / 2
    eye = centre + np.array([2.6, 1.5, 3.1])
    cam = scenes.look_at_camera(eye, centre, 40.0, float(np.linalg.norm(eye - centre)), 0.02)
    return svo, cam, dict(scene="dragon", grid=res, levels=int(info.levels), voxels=int(info.numberOfVoxels), size=[W, H]), build_ms


def step_pyramid(mv, args, res):
    svo, _, base, build_ms = build_dragon(mv, res)
    ms, ts = bk.timed_async(mv, lambda: svo.lod_prepare(), args.reps, args.warmup)
    return [dict(op="lod_prepare", ms=ms, all_ms=ts, lod_bytes=svo.lod_bytes(), traversal_bytes=int(svo.traversal_bytes()), voxel_list_bytes=base["voxels"] * 16,
                 build_ms=build_ms, **base)]


def step_rays(mv, args, res, which):
    svo, cam, base, _ = build_dragon(mv, res)
    ro, rd = pixel_rays(cam)
    n = len(ro)
    dev = [mv.DeviceArray.from_host(np.ascontiguousarray(a)) for a in (ro[:, 0], ro[:, 1], ro[:, 2], rd[:, 0], rd[:, 1], rd[:, 2])]
    t, nm, lv, de = mv.DeviceArray(n, np.float32), mv.DeviceArray(n, np.int32), mv.DeviceArray(n, np.uint32), mv.DeviceArray(n, np.uint32)
    inf = mv.DeviceArray.from_host(np.full(n, np.inf, np.float32))
    yardstick = lambda: svo.intersect_range_device(n, *dev, None, inf, t, nm, None, de)
    if which == "yardstick":
        ms, ts = bk.timed_async(mv, yardstick, args.reps, args.warmup)
        return [dict(op="trace_batch_range", tMax="+inf", ms=ms, all_ms=ts, descents_per_ray=float(de.to_host().mean()), hits=int((t.to_host() != MAXF).sum()), **base)]
    yardstick()
    mv.synchronize()
    yard_t, yard_de = t.to_host(), de.to_host()
    zero = mv.DeviceArray.from_host(np.zeros(n, np.float32))
    rows = []
    for scale in SCALES:
        cone_b = f32(scale) * ((f32(2.0) * f32(cam[12])) / f32(H))
        db = mv.DeviceArray.from_host(np.full(n, cone_b, np.float32))
        ms, ts = bk.timed_async(mv, lambda: svo.intersect_cone_device(n, *dev, zero, db, t, nm, lv, None, None, None, de), args.reps, args.warmup)
        got_t, got_de, got_lv = t.to_host(), de.to_host(), lv.to_host()
        rows.append(dict(op="trace_batch_cone", lodScale=scale, ms=ms, all_ms=ts, descents_per_ray=float(got_de.mean()), descents_per_ray_unlimited=float(yard_de.mean()),
                         hits=int((got_t != MAXF).sum()), level_histogram=np.bincount(got_lv, minlength=base["levels"] + 1).tolist(),
                         never_more_descents=bool((got_de <= yard_de).all()), equal_to_yardstick=bool(np.array_equal(got_t, yard_t)) if scale == 0.0 else None, **base))
        del db
    return rows


def step_render(mv, args, res):
    svo, cam, base, _ = build_dragon(mv, res)
    svo.lod_prepare()
    rgba = mv.DeviceArray((W * H, 4), np.uint8)
    ms, ts = bk.timed_async(mv, lambda: svo.render_device(cam, W, H, True, rgba), args.reps, args.warmup)
    rows = [dict(op="render_primary", ms=ms, all_ms=ts, **base)]
    lib = mv.lib()
    cam32 = np.ascontiguousarray(cam, np.float32)
    for scale in SCALES:
        def render():
            if lib.mvrt_render_primary_lod(svo._h, cam32.ctypes.data, W, H, float(scale), 1, rgba.ptr, None, None, None, None, None) != 0:
                raise RuntimeError(lib.mvrt_last_error().decode())
        ms, ts = bk.timed_async(mv, render, args.reps, args.warmup)
        rows.append(dict(op="render_primary_lod", lodScale=scale, ms=ms, all_ms=ts, **base))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", default="2048,8192")
    ap.add_argument("--steps", default=",".join(STEPS))
    bk.add_step_args(ap, reps=5, warmup=1, step_timeout=240, out=os.path.join(bk.ROOT, "profiles", "lod_cone_bench.json"))
    args = ap.parse_args()
    if args.step:
        import massivevoxelraytracing_amd as mv
        mv.set_device(0)
        step, res = args.step.split(":")
        for row in step_pyramid(mv, args, int(res)) if step == "pyramid" else step_render(mv, args, int(res)) if step == "render" else step_rays(mv, args, int(res), step):
            bk.emit(row)
        return 0
    for step in args.steps.split(","):
        if step not in STEPS:
            ap.error("unknown step " + step)
    steps = [s + ":" + g for g in args.grids.split(",") for s in args.steps.split(",")]
    return bk.run_steps(__file__, steps, lambda s: bk.flags(args, "reps", "warmup"), args.step_timeout, args.out, echo=bk.brief)[1]


if __name__ == "__main__":
    sys.exit(main())
