#!/usr/bin/env python3
"""usage: tools/upload_walk_bench.py [--scenes dragon[:grid],rtcamp[:grid]] [--reps 10] [--warmup 2] [--no-pt] [--kernel-stats DIR] [--out profiles/upload_walk_bench.json]

Cost of walking an uploaded octree (mvrt_svo_walk_voxels, mvrt_svo_rebuild) on the two uploads DESIGN.md 5.6 measures: the dragon stand-in's 2048^3 DAG and
the rtcamp stand-in's 4096^3 DAG, each built on the GPU, downloaded and uploaded again (an upload keeps no Morton codes, so it is walked from the root).
  walk      the sizing call plus the fill into device arrays allocated before the clock starts
  rebuild   mvrt_svo_rebuild( 0 ) of a fresh upload (the upload itself is outside the clock)
  build     mvrt_svo_build_voxels of the walked list (device arrays), flags 0: what a user with the list in hand would pay
Median of --reps calls after --warmup calls; host clock around each call (every call ends in a synchronise).
The last-level emit's algorithmic bytes (per parent of voxels: 16 B frontier entry, 8 B offset, one 64-byte node line; per voxel: 12 B written) stand next
to the 8 TB/s HBM peak once a kernel trace of its own gives the kernel's time.  The parents are PATHS: a DAG's node is the parent on many of them, so a second
figure counts every node line once at most (min(parents, nodes) lines), the least HBM can have served if the caches kept every shared line:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/upload_walk_bench.py --scenes dragon --reps 3 --no-pt
and --kernel-stats DIR in the plain run (one scene per trace, since the statistics are per kernel name; traces of several scenes go to DIR/<scene>).
Once, on the dragon: path-tracer ms per 16-spp step at 1920x1080 on the upload before and after rebuild, the two alternated in one process -- what the cell
index is worth to an upload."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

import numpy as np

import benchkit as bk
import massivevoxelraytracing_amd as mv
from massivevoxelraytracing_amd import scenes

UPLOADS = dict(dragon=2048, rtcamp=4096)
HBM_PEAK = 8.0e12


def last_emit_stats(directory):
    """the last-level emit kernels (kWalkEmit<*, true>) of a rocprofv3 --kernel-trace --stats directory"""
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            name = r.get("Name", "")
            if "kWalkEmit" in name and ("true>" in name.replace(" ", "") or "Lb1EEE" in name):
                return {"name": name, "calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3, "max_us": float(r["MaxNs"]) / 1e3}
    return None


def pt_before_after(nodes, attrs, info, reps, frames=4, frame_steps=4):
    W, H = 1920, 1080
    pt = mv.PathTracer()
    pt.setup(None)
    pt.resizeFrameBufferIfNeeded(None, W, H)
    hdr = os.path.join(bk.ROOT, "tests", "golden", "monks_forest_s.hdr")
    pt.loadHDRI(None, hdr, hdr)
    svo = pt.m_intersectorOctreeGPU
    lo, hi = np.array(info.lower[:]), np.array(info.upper[:])
    centre = (lo + hi) / 2
    eye = centre + np.array([2.6, 1.5, 3.1])  # bench.py's dragon camera
    cam = scenes.look_at_camera(eye, centre, 40.0, float(np.linalg.norm(eye - centre)), 0.02)

    def run(k):
        for _ in range(k):
            pt.clearFrameBuffer(None)
            for _ in range(frame_steps):
                pt.step(None, cam)
            pt.join(None)
            mv.synchronize()

    def measure():
        run(2)
        t0 = time.perf_counter()
        run(frames)
        return (time.perf_counter() - t0) * 1e3 / (frames * frame_steps)

    up, re = [], []
    for _ in range(reps):
        svo.upload(nodes, attrs, info.lower[:], info.dps, info.gridRes, info.hasEmission, embeddedMask=bool(info.embeddedMask))
        up.append(measure())
        svo.rebuild(0)
        re.append(measure())
    return {"op": "pt_ms_per_16spp_step", "width": W, "height": H, "uploaded": up, "rebuilt": re, "median_uploaded": statistics.median(up),
            "median_rebuilt": statistics.median(re), "rebuilt_over_uploaded": statistics.median(re) / statistics.median(up)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=lambda text: bk.parse_scenes(text, UPLOADS), default="dragon,rtcamp")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pt-reps", type=int, default=3)
    ap.add_argument("--no-pt", action="store_true")
    ap.add_argument("--kernel-stats", metavar="DIR", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    mv.set_device(0)
    rows = []

    def emit(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    for name, res in args.scenes:
        built, origin, dps = bk.built(mv, name, res)
        info = built.info()
        nodes, attrs, morton = built.download(want_morton=True)
        n_parents = int(np.unique(morton >> np.uint64(3)).size)
        del built, morton
        args_up = (nodes, attrs, origin, dps, res, info.hasEmission)
        up = mv.IntersectorOctreeGPU()
        up.upload(*args_up, embeddedMask=bool(info.embeddedMask))
        n = up.walk_voxels_device()
        base = dict(scene=name, grid=res, nodes=info.numberOfNodes, voxels=info.numberOfVoxels, paths=n, levels=info.levels)
        xyz, vi, at = mv.DeviceArray((n, 3), np.uint32), mv.DeviceArray(n, np.uint32), mv.DeviceArray((n, 8), np.uint8)

        def walk():
            up.walk_voxels_device(up.walk_voxels_device(), xyz, vi, at)

        ms, ts = bk.timed(mv, walk, args.reps, args.warmup)
        emit(op="walk_voxels", ms=ms, all_ms=ts, **base)
        ms, ts = bk.timed(mv, lambda: up.walk_voxels_device(), args.reps, args.warmup)
        emit(op="walk_voxels_sizing_call", ms=ms, all_ms=ts, **base)
        b = n_parents * (16 + 8 + 64) + n * 12
        b_once = n_parents * (16 + 8) + min(n_parents, info.numberOfNodes) * 64 + n * 12
        row = dict(op="last_level_emit", parents=n_parents, algorithmic_bytes=b, bytes_with_each_line_once=b_once, ms_at_hbm_peak=b / HBM_PEAK * 1e3, **base)
        if args.kernel_stats:
            per_scene = os.path.join(args.kernel_stats, name)  # DIR/<scene> where there is one trace per scene
            ks = last_emit_stats(per_scene if os.path.isdir(per_scene) else args.kernel_stats)
            if ks:
                row.update(kernel=ks, bytes_per_s=b / (ks["avg_us"] * 1e-6), of_hbm_peak=b / (ks["avg_us"] * 1e-6) / HBM_PEAK,
                           each_line_once_bytes_per_s=b_once / (ks["avg_us"] * 1e-6), each_line_once_of_hbm_peak=b_once / (ks["avg_us"] * 1e-6) / HBM_PEAK)
        emit(**row)
        target = mv.IntersectorOctreeGPU()
        ms, ts = bk.timed(mv, lambda: target.rebuild(0), args.reps, args.warmup, before=lambda: target.upload(*args_up, embeddedMask=bool(info.embeddedMask)))
        emit(op="rebuild", ms=ms, all_ms=ts, **base)
        ms, ts = bk.timed(mv, lambda: target.build_voxels(xyz, at, origin=origin, dps=dps, gridRes=res, flags=0), args.reps, args.warmup)
        emit(op="build_voxels_of_the_walked_list", ms=ms, all_ms=ts, **base)
        del target, up, xyz, vi, at
        if name == "dragon" and not args.no_pt:
            emit(scene=name, grid=res, **pt_before_after(nodes, attrs, info, args.pt_reps))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")
    for r in rows:
        if "ms" in r:
            print("%-7s %5d %-32s %9d paths %9.2f ms" % (r["scene"], r["grid"], r["op"], r["paths"], r["ms"]), file=sys.stderr)


if __name__ == "__main__":
    main()
