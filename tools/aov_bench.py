#!/usr/bin/env python3
"""Cost of the first-hit feature buffers (mvrt_pt_set_aovs) on the headline workload: dragon stand-in 2048^3, 1920x1080, 64-spp frames.

    python3 tools/aov_bench.py [--reps 5] [--frames 6] [--out profiles/aov_bench.json] [--kernel-stats DIR]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/aov_bench.py --profile-run     (a run of its own)

The plain run renders frames (clear, 4 steps, join, device synchronise) with the feature buffers off and on, alternated in ONE process after a warm-up of each, and
reports ms per step from a host clock around whole frames.  --profile-run renders a few frames with the buffers on, one step per pass on one stream, so that a
kernel trace shows the two new kernels un-overlapped; --kernel-stats DIR adds their times from that trace, against their algorithmic bytes (computed here from the
frame shape and the counted hits) at the streaming-read ceiling measured on the box (profiles/r02_stream_read.txt)."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAM_READ_CEILING_GBS = 6100.0  # tools/calib/stream_read.hip, profiles/r02_stream_read.txt


def algorithmic_bytes(pixels, hits_per_step):
    """per step.  reduce: per pixel 16 x (4 hitT + 8 hitPath + 1 hitN + 12 direction) B of records read and 32 B of partial sums written, 8 B of attributes per
    hit; add: 32 B of partial sums read, 2 x (16 B read + 16 B written) of the two buffers (one step per pass; merged steps share the read-modify-write)"""
    return {"reduce": pixels * (16 * 25 + 32) + hits_per_step * 8, "add": pixels * (32 + 64)}


def kernel_stats(directory):
    rows = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            name = r.get("Name", "")
            for k in ("kPtAovReduce", "kPtAovAccumulate", "kPtAccumulate", "kPtGenerate"):
                if name.startswith(k) or (" " + k) in name:
                    rows[k] = {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3, "max_us": float(r["MaxNs"]) / 1e3}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="dragon")
    ap.add_argument("--grid-res", type=int, default=2048)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frame-steps", type=int, default=4)
    ap.add_argument("--frames", type=int, default=6, help="timed frames per measurement")
    ap.add_argument("--reps", type=int, default=5, help="measurements of each setting, alternated")
    ap.add_argument("--detail", type=float, default=1.0)
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--kernel-stats", metavar="DIR", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import massivevoxelraytracing_amd as mv
    from massivevoxelraytracing_amd import scenes
    mv.lib()
    mv.set_device(0)
    verts, cols, emis = scenes.SCENES[args.scene](args.detail)
    origin, dps = scenes.bounding_grid(verts, args.grid_res)
    W, H = args.width, args.height
    pt = mv.PathTracer()
    pt.setup(None)
    pt.resizeFrameBufferIfNeeded(None, W, H)
    hdr = os.path.join(ROOT, "tests", "golden", "monks_forest_s.hdr")
    pt.loadHDRI(None, hdr, hdr)
    pt.updateScene(verts, cols, emis, None, origin, dps, args.grid_res)
    info = pt.m_intersectorOctreeGPU.info()
    lo, hi = np.array(info.lower[:]), np.array(info.upper[:])
    centre = (lo + hi) / 2
    eye = centre + np.array([2.6, 1.5, 3.1])  # bench.py's dragon camera
    cam = scenes.look_at_camera(eye, centre, 40.0, float(np.linalg.norm(eye - centre)), 0.02)

    def frames(k):
        for _ in range(k):
            pt.clearFrameBuffer(None)
            for _ in range(args.frame_steps):
                pt.step(None, cam)
            pt.join(None)
            mv.synchronize()

    if args.profile_run:
        pt.set_pipeline_depth(1)
        pt.set_batch_steps(1)
        pt.set_split_small_passes(False)
        pt.clearFrameBuffer(None)
        pt.set_aovs(True)
        frames(3)
        print(json.dumps({"profile_run": True, "steps": 3 * args.frame_steps}))
        return

    def measure(on):
        pt.clearFrameBuffer(None)
        pt.set_aovs(on)  # reallocates the path state: outside the timed region
        frames(2)        # warm-up of this setting (also tells the library the frame length)
        mv.synchronize()
        t0 = time.perf_counter()
        frames(args.frames)
        return (time.perf_counter() - t0) * 1e3 / (args.frames * args.frame_steps)

    off, on = [], []
    for _ in range(args.reps):
        off.append(measure(False))
        on.append(measure(True))
    hits_per_step = float(pt.read_aov(pt.AOV_ALBEDO)[: W * H, 3].astype(np.float64).sum()) / args.frame_steps  # the last frame's primary hits
    b = algorithmic_bytes(W * H, hits_per_step)
    floor_ms = {k: v / (STREAM_READ_CEILING_GBS * 1e9) * 1e3 for k, v in b.items()}
    out = {
        "workload": "%s stand-in %d^3, %dx%d, frames of %d steps, %d timed frames per measurement, %d measurements of each setting alternated in one process" % (
            args.scene, args.grid_res, W, H, args.frame_steps, args.frames, args.reps),
        "device": mv.device_name(),
        "ms_per_step_off": [round(x, 4) for x in off], "ms_per_step_on": [round(x, 4) for x in on],
        "median_off": round(statistics.median(off), 4), "median_on": round(statistics.median(on), 4),
        "spread_off": round(max(off) - min(off), 4), "spread_on": round(max(on) - min(on), 4),
        "overhead_percent": round(100.0 * (statistics.median(on) / statistics.median(off) - 1.0), 2),
        "primary_hits_per_step": hits_per_step, "hit_share": round(hits_per_step / (W * H * 16), 4),
        "algorithmic_bytes_per_step": b, "floor_ms_at_streaming_ceiling": {k: round(v, 4) for k, v in floor_ms.items()}, "ceiling_GBs": STREAM_READ_CEILING_GBS,
    }
    if args.kernel_stats:
        ks = kernel_stats(args.kernel_stats)
        out["kernels"] = ks
        for k, name in (("reduce", "kPtAovReduce"), ("add", "kPtAovAccumulate")):
            if name in ks:
                out.setdefault("share_of_ceiling", {})[k] = round(floor_ms[k] * 1e3 / ks[name]["avg_us"], 3)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
