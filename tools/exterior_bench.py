#!/usr/bin/env python3
"""usage: tools/exterior_bench.py [--scenes dragon[:grid],tunnel[:grid]] [--reps 10] [--warmup 2] [--step-timeout 360] [--baseline-lib path/to/libmvrt_hip.so]
                                  [--rounds 2] [--out profiles/exterior_bench.json] [--no-fill-route]

Cost of the exterior masks next to what they replace, on the procedural stand-ins (dragon 2048^3, tunnel 4096^3):
  masks           mvrt_svo_surface_masks into a device array
  exterior        mvrt_svo_surface_exterior_masks into a device array: linear keys + radix sort + unions + flatten, the masks kernel, one pass that clears bits
  exterior_count  the same with masksDev NULL (counts only)
  count           mvrt_svo_enclosed_cells, the sizing call: what a caller without this feature pays to learn which cells are enclosed
  quads           mvrt_svo_surface_quads into device arrays
  quads_masked    mvrt_svo_surface_quads_masked with the exterior masks into device arrays
  fill_route      once per scene where the fill fits: mvrt_svo_fill_enclosed followed by mvrt_svo_surface_masks, the only route to the same faces without this
                  feature (the octree is rebuilt from its voxel list before every call, outside the clock; at most 3 calls after 1 warm-up)
Median of --reps calls after --warmup calls; host clock around each call (every call blocks until its counts are back).  Output arrays are allocated before the
clock starts.  With --baseline-lib the steps masks, count and quads (and the fill route) also run on that build of the library -- the parent commit's, say -- in
the same job: rows with lib = "baseline", the two builds taking turns, --rounds times each (baseline, this, baseline, this: one process per turn, so the
spread from one process to the next shows beside the spread of the calls of one process).  The yardstick for "the refactor costs the existing calls nothing" is
the spread of the baseline's own calls.
Every step runs in a child process of its own under --step-timeout seconds; a step that fails, is killed or runs out of time ends the run: nothing more is
started on the GPU behind it."""
import argparse
import ctypes
import os
import sys

import numpy as np

import benchkit as bk


def step(args):
    """one child process: prints one JSON row per measurement"""
    import massivevoxelraytracing_amd as mv
    have = ctypes.CDLL(mv.LIB_PATH)
    for name in [s for s in mv.SIGNATURES if not hasattr(have, s)]:  # an older build of the library: bind what it has
        del mv.SIGNATURES[name]
    new = "mvrt_svo_surface_exterior_masks" in mv.SIGNATURES
    mv.set_device(0)
    name, res, op, lib_name, rnd = args.step.split(":")
    res = int(res)
    svo, origin, dps = bk.built(mv, name, res)
    n_vox = svo.info().numberOfVoxels
    n_cells, n_regions = svo.enclosed_cells_device()
    n_plain = svo.surface_masks_device()
    base = dict(scene=name, grid=res, voxels=n_vox, nCells=n_cells, nRegions=n_regions, nFacesPlain=n_plain, lib=lib_name, round=int(rnd))

    def run(op, fn, **kw):
        ms, ts = bk.timed(mv, fn, args.reps, args.warmup)
        bk.emit(base, op=op, ms=ms, all_ms=ts, **kw)

    if op == "masks":
        masks = mv.DeviceArray(n_vox, np.uint8)
        run("masks", lambda: svo.surface_masks_device(masks))
        run("count", svo.enclosed_cells_device)
        if new:
            n_ext, n_hidden = svo.surface_exterior_masks_device()
            run("exterior", lambda: svo.surface_exterior_masks_device(masks), nFaces=n_ext, nHidden=n_hidden)
            run("exterior_count", svo.surface_exterior_masks_device, nFaces=n_ext, nHidden=n_hidden)
    elif op == "quads":
        fv, fd, pos = mv.DeviceArray(n_plain, np.uint32), mv.DeviceArray(n_plain, np.uint8), mv.DeviceArray((n_plain, 12), np.float32)
        run("quads", lambda: svo.surface_quads_device(n_plain, fv, fd, pos), nFaces=n_plain)
        if new:
            masks = mv.DeviceArray(n_vox, np.uint8)
            n_ext, n_hidden = svo.surface_exterior_masks_device(masks)
            run("quads_masked", lambda: svo.surface_quads_device(n_ext, fv, fd, pos, masks=masks), nFaces=n_ext, nHidden=n_hidden)
    elif op == "fill":
        if n_cells == 0 or n_cells > args.max_cells or n_cells + n_vox >= (1 << 32) - 1:
            bk.emit(base, op="fill_route", skipped="no cells" if n_cells == 0 else "%d cells are more than the fill is given here" % n_cells)
            return
        xyz, attrs = bk.snapshot(mv, svo)
        masks = mv.DeviceArray(n_vox + n_cells, np.uint8)
        faces = []

        def route():
            svo.fill_enclosed()
            faces.append(svo.surface_masks_device(masks))

        ms, ts = bk.timed(mv, route, args.reps, args.warmup, before=lambda: svo.build_voxels(xyz, attrs, origin=origin, dps=dps, gridRes=res))
        assert len(set(faces)) == 1
        bk.emit(base, op="fill_route", ms=ms, all_ms=ts, nFaces=faces[0], voxels_after=svo.info().numberOfVoxels)


def line(r):
    what = "%9.2f ms  (%.2f .. %.2f)" % (r["ms"], min(r["all_ms"]), max(r["all_ms"])) if "ms" in r else r.get("skipped") or r.get("failed")
    return "%-7s %5s %-9s %s %-15s %10s voxels %11s faces  %s" % (r.get("scene", r.get("step")), r.get("grid", ""), r.get("lib", ""), r.get("round", ""), r.get("op", ""), r.get("voxels", ""),
                                                               r.get("nFaces", r.get("nFacesPlain", "")), what)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=bk.parse_scenes, default="dragon,tunnel")
    ap.add_argument("--max-cells", type=int, default=1 << 30)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--no-fill-route", action="store_true")
    bk.add_step_args(ap, reps=10, warmup=2, step_timeout=360)
    args = ap.parse_args()
    if args.step:
        return step(args)
    libs = ["this"] + (["baseline"] if args.baseline_lib else [])
    steps = []  # scene:grid:op:lib:round
    for scene in args.scenes:
        for op in ("masks", "quads"):  # the two builds of the library next to each other, step by step
            steps += ["%s:%d:%s:%s:%d" % (*scene, op, lib, r) for r in range(args.rounds) for lib in reversed(libs)]
        if not args.no_fill_route:
            steps.append("%s:%d:fill:%s:0" % (*scene, libs[-1]))

    def child_args(s):
        fill = s.split(":")[2] == "fill"  # seconds per call, and bimodal: a few calls show the order of magnitude
        return ["--reps", str(min(args.reps, 3) if fill else args.reps), "--warmup", str(min(args.warmup, 1) if fill else args.warmup)] + bk.flags(args, "max_cells")

    lib_of = lambda s: s.split(":")[3]
    rows, rc = bk.run_steps(__file__, steps, child_args, args.step_timeout, args.out, failed_fields=lambda s: dict(lib=lib_of(s)),
                            env_for=lambda s: dict(MVRT_LIB=os.path.abspath(args.baseline_lib)) if lib_of(s) == "baseline" else None)
    bk.print_table(rows, line)
    return rc


if __name__ == "__main__":
    sys.exit(main())
