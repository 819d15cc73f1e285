#!/usr/bin/env python3
"""usage: tools/exterior_bench.py [--scenes dragon,tunnel] [--reps 10] [--warmup 2] [--step-timeout 360] [--baseline-lib path/to/libmvrt_hip.so]
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
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRID = {"dragon": 2048, "tunnel": 4096}


def timed(mv, fn, reps, warmup, before=None):
    ts = []
    for i in range(warmup + reps):
        if before:
            before()
        mv.synchronize()
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), ts


def step(args):
    """one child process: prints one JSON row per measurement"""
    import massivevoxelraytracing_amd as mv
    from massivevoxelraytracing_amd import scenes
    have = ctypes.CDLL(mv.LIB_PATH)
    for name in [s for s in mv.SIGNATURES if not hasattr(have, s)]:  # an older build of the library: bind what it has
        del mv.SIGNATURES[name]
    new = "mvrt_svo_surface_exterior_masks" in mv.SIGNATURES
    mv.set_device(0)
    name, op = args.step.split(":")
    res = GRID[name]
    verts, cols, emis = scenes.SCENES[name](1.0)
    origin, dps = scenes.bounding_grid(verts, res)
    svo = mv.IntersectorOctreeGPU()
    svo.build(verts, cols, emis, None, origin, dps, res)
    n_vox = svo.info().numberOfVoxels
    n_cells, n_regions = svo.enclosed_cells_device()
    n_plain = svo.surface_masks_device()
    base = dict(scene=name, grid=res, voxels=n_vox, nCells=n_cells, nRegions=n_regions, nFacesPlain=n_plain, lib=args.lib_name, round=args.round)

    def emit(**kw):
        print(json.dumps(dict(kw, **base)), flush=True)

    def run(op, fn, **kw):
        ms, ts = timed(mv, fn, args.reps, args.warmup)
        emit(op=op, ms=ms, all_ms=ts, **kw)

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
            emit(op="fill_route", skipped="no cells" if n_cells == 0 else "%d cells are more than the fill is given here" % n_cells)
            return
        xyz, attrs = mv.DeviceArray((n_vox, 3), np.uint32), mv.DeviceArray((n_vox, 8), np.uint8)
        mv._check(mv.lib().mvrt_svo_read_voxels(svo._h, xyz.ptr, attrs.ptr, None))
        masks = mv.DeviceArray(n_vox + n_cells, np.uint8)
        faces = []

        def route():
            svo.fill_enclosed()
            faces.append(svo.surface_masks_device(masks))

        ms, ts = timed(mv, route, args.reps, args.warmup, before=lambda: svo.build_voxels(xyz, attrs, origin=origin, dps=dps, gridRes=res))
        assert len(set(faces)) == 1
        emit(op="fill_route", ms=ms, all_ms=ts, nFaces=faces[0], voxels_after=svo.info().numberOfVoxels)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="dragon,tunnel")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=360)
    ap.add_argument("--max-cells", type=int, default=1 << 30)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-fill-route", action="store_true")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--lib-name", default="this", help=argparse.SUPPRESS)
    ap.add_argument("--round", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        return step(args)
    libs = [("this", None)] + ([("baseline", os.path.abspath(args.baseline_lib))] if args.baseline_lib else [])
    steps = []
    for s in args.scenes.split(","):
        for op in ("masks", "quads"):  # the two builds of the library next to each other, step by step
            steps += [(s + ":" + op, lib, r) for r in range(args.rounds) for lib in reversed(libs)]
        if not args.no_fill_route:
            steps.append((s + ":fill", libs[-1], 0))
    rows, rc = [], 0
    for s, (lib_name, lib_path), rnd in steps:
        fill = s.endswith(":fill")  # seconds per call, and bimodal: a few calls show the order of magnitude
        cmd = [sys.executable, os.path.abspath(__file__), "--step", s, "--lib-name", lib_name, "--round", str(rnd), "--reps", str(min(args.reps, 3) if fill else args.reps),
               "--warmup", str(min(args.warmup, 1) if fill else args.warmup), "--max-cells", str(args.max_cells)]
        env = dict(os.environ)
        if lib_path:
            env["MVRT_LIB"] = lib_path
        print("step", s, lib_name, "round", rnd, flush=True)
        try:
            out = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=args.step_timeout, env=env)
        except subprocess.TimeoutExpired:
            rows.append(dict(step=s, lib=lib_name, failed="no result within %d s" % args.step_timeout))
            rc = 1
            break
        for line in out.stdout.decode().splitlines():
            if line.startswith("{"):
                rows.append(json.loads(line))
                print(line, flush=True)
        if out.returncode != 0:
            rows.append(dict(step=s, lib=lib_name, failed="exit status %d" % out.returncode))
            rc = 1
            break  # nothing more is started on the GPU behind a step that failed
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
    for r in rows:
        what = "%9.2f ms  (%.2f .. %.2f)" % (r["ms"], min(r["all_ms"]), max(r["all_ms"])) if "ms" in r else r.get("skipped") or r.get("failed")
        print("%-7s %5s %-9s %s %-15s %10s voxels %11s faces  %s" % (r.get("scene", r.get("step")), r.get("grid", ""), r.get("lib", ""), r.get("round", ""), r.get("op", ""), r.get("voxels", ""),
                                                                 r.get("nFaces", r.get("nFacesPlain", "")), what), file=sys.stderr)
    return rc


if __name__ == "__main__":
    sys.exit(main())
