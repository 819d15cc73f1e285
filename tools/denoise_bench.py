#!/usr/bin/env python3
"""Cost of the luminance moments (mvrt_pt_set_moments) and of the denoiser (mvrt_pt_denoise) on the headline workload: dragon stand-in 2048^3, 1920x1080, 64-spp frames.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/denoise_bench.py --profile-run     (a run of its own, first)
    python3 tools/denoise_bench.py --kernel-stats DIR --out profiles/denoise_bench.json --csv profiles/denoise_kernel_stats.csv

Each GPU step under a time limit of its own, chained so that nothing starts after a failure:

    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/denoise_bench.py --profile-run &&
    timeout -k 10 300 python3 tools/denoise_bench.py --kernel-stats DIR --out profiles/denoise_bench.json --csv profiles/denoise_kernel_stats.csv

The plain run measures, in ONE process: (a) ms per step of frames (clear, 4 steps, join, device synchronise) with the moments off and on, alternated, --reps measurements
of --frames frames each after a warm-up of each setting (host clock around whole frames; the spread of the off runs is the yardstick); (b) the time of one
mvrt_pt_denoise with the default parameters on the last 64-spp frame: --denoise-calls calls between two device synchronises, after a warm-up.  It also states the
one comparison that is not a measurement: a denoise must cost less than one 16-spp step of the same run.  --profile-run renders one frame with everything on, one
step per pass on one stream, and denoises it a few times, so that a kernel trace shows the new kernels un-overlapped; --kernel-stats DIR adds their times from that
trace against their algorithmic bytes (computed here from the frame shape and the counted hit pixels) at the streaming-read ceiling measured on the box
(profiles/r02_stream_read.txt)."""
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
KERNELS = ("kPtMoments", "kDenoisePrepare", "kDenoiseAtrous<false>", "kDenoiseAtrous<true>", "kPtAccumulate", "kPtAovAccumulate")


def algorithmic_bytes(pixels, hit_pixels):
    """compulsory traffic per launch.  moments (one step per pass): 16 samples x 12 B of radiance read, 16 B read + 16 B written of the buffer.  prepare: a pixel with a hit
    reads the four 16-byte inputs and writes 36 B of records; a pixel without one (sky, no samples) returns after color and albedo (32 B) and writes the records and its
    output (52 B).  a-trous: per pixel the 36 B of records read ONCE (the 25-fold re-read is cache traffic, not compulsory), 16 B written per filtered pixel; the last
    iteration also reads albedo and color of the filtered pixels (32 B)"""
    sky = pixels - hit_pixels
    return {"kPtMoments": pixels * (16 * 12 + 32), "kDenoisePrepare": hit_pixels * (64 + 36) + sky * (32 + 52), "kDenoiseAtrous<false>": pixels * 36 + hit_pixels * 16,
            "kDenoiseAtrous<true>": pixels * 36 + hit_pixels * (16 + 32)}


def kernel_stats(directory):
    rows = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            name = r.get("Name", "")
            for k in KERNELS:
                base, _, targ = k.partition("<")
                if (name.startswith(base) or (" " + base) in name) and (not targ or ("<" + targ) in name.replace("(bool)0", "false").replace("(bool)1", "true")):
                    rows[k] = {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3, "max_us": float(r["MaxNs"]) / 1e3,
                               "total_us": float(r["TotalDurationNs"]) / 1e3 if "TotalDurationNs" in r else None}
    return rows


def per_stride_us(directory, iterations=5):
    """mean time of the a-trous launch of each stride, from the dispatches of the kernel trace in start order (a default denoise is `iterations` launches, strides 1, 2, 4, ...)"""
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            if "kDenoiseAtrous" in r.get("Kernel_Name", ""):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    rows.sort()
    if not rows or len(rows) % iterations:
        return None
    out = []
    for i in range(iterations):
        d = [(e - b) / 1e3 for b, e in rows[i::iterations]]
        out.append({"stride": 1 << i, "avg_us": round(sum(d) / len(d), 2), "min_us": round(min(d), 2), "max_us": round(max(d), 2)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="dragon")
    ap.add_argument("--grid-res", type=int, default=2048)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frame-steps", type=int, default=4)
    ap.add_argument("--frames", type=int, default=6, help="timed frames per measurement")
    ap.add_argument("--reps", type=int, default=5, help="measurements of each setting, alternated")
    ap.add_argument("--denoise-calls", type=int, default=50, help="timed denoise calls between two device synchronises (at least 50)")
    ap.add_argument("--detail", type=float, default=1.0)
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--denoise-only", action="store_true", help="skip (a): only the time of mvrt_pt_denoise (A/B of two builds of the library through MVRT_LIB)")
    ap.add_argument("--kernel-stats", metavar="DIR", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--csv", default=None)
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
        pt.set_moments(True)
        frames(2)
        for _ in range(10):
            pt.denoise(None)
        mv.synchronize()
        print(json.dumps({"profile_run": True, "steps": 2 * args.frame_steps, "denoise_calls": 10}))
        return

    def measure(on):
        pt.clearFrameBuffer(None)
        pt.set_moments(on)  # reallocates the path state: outside the timed region
        frames(2)           # warm-up of this setting (also tells the library the frame length)
        mv.synchronize()
        t0 = time.perf_counter()
        frames(args.frames)
        return (time.perf_counter() - t0) * 1e3 / (args.frames * args.frame_steps)

    off, on = [], []
    for _ in range(1 if args.denoise_only else args.reps):
        off.append(measure(False))
        if not args.denoise_only:
            on.append(measure(True))
    if args.denoise_only:
        on = off
    # (b) the denoiser on a 64-spp frame of the same scene
    pt.clearFrameBuffer(None)
    pt.set_aovs(True)
    pt.set_moments(True)
    frames(1)
    for _ in range(5):
        pt.denoise(None)
    mv.synchronize()
    calls = max(50, args.denoise_calls)
    t0 = time.perf_counter()
    for _ in range(calls):
        pt.denoise(None)
    mv.synchronize()
    denoise_ms = (time.perf_counter() - t0) * 1e3 / calls
    hit_pixels = int((pt.read_aov(pt.AOV_ALBEDO)[: W * H, 3] > 0).sum())
    b = algorithmic_bytes(W * H, hit_pixels)
    floor_us = {k: v / (STREAM_READ_CEILING_GBS * 1e9) * 1e6 for k, v in b.items()}
    step_ms = statistics.median(off)
    from massivevoxelraytracing_amd import build as B
    out = {
        "library_source_digest": B.source_digest(),  # the build these figures belong to (bench.py's rule for committed profiles)
        "workload": "%s stand-in %d^3, %dx%d, frames of %d steps, %d timed frames per measurement, %d measurements of each setting alternated in one process" % (
            args.scene, args.grid_res, W, H, args.frame_steps, args.frames, args.reps),
        "device": mv.device_name(),
        "moments": {"ms_per_step_off": [round(x, 4) for x in off], "ms_per_step_on": [round(x, 4) for x in on], "median_off": round(statistics.median(off), 4),
                    "median_on": round(statistics.median(on), 4), "spread_off": round(max(off) - min(off), 4), "spread_on": round(max(on) - min(on), 4),
                    "difference_ms": round(statistics.median(on) - statistics.median(off), 4), "overhead_percent": round(100.0 * (statistics.median(on) / statistics.median(off) - 1.0), 2)},
        "denoise": {"ms_per_call": round(denoise_ms, 4), "calls_between_synchronises": calls, "parameters": "defaults (5 iterations)", "after": "%d-spp frame" % (16 * args.frame_steps),
                    "hit_pixel_share": round(hit_pixels / (W * H), 4), "scratch_bytes": mv.denoise_scratch_bytes(W, H),
                    "one_16spp_step_ms_same_run": round(step_ms, 4), "cheaper_than_one_step": bool(denoise_ms < step_ms)},
        "algorithmic_bytes_per_launch": b, "floor_us_at_streaming_ceiling": {k: round(v, 2) for k, v in floor_us.items()}, "ceiling_GBs": STREAM_READ_CEILING_GBS,
    }
    if args.kernel_stats:
        ks = kernel_stats(args.kernel_stats)
        out["kernels"] = ks
        out["share_of_ceiling"] = {k: round(floor_us[k] / ks[k]["avg_us"], 3) for k in floor_us if k in ks}
        out["atrous_per_stride"] = per_stride_us(args.kernel_stats)
        if args.csv:
            with open(args.csv, "w", newline="") as f:
                wr = csv.writer(f)
                wr.writerow(["kernel", "calls", "avg_us", "min_us", "max_us", "algorithmic_bytes", "floor_us_at_%g_GBs" % STREAM_READ_CEILING_GBS, "share_of_ceiling"])
                for k in KERNELS:
                    if k in ks:
                        wr.writerow([k, ks[k]["calls"], round(ks[k]["avg_us"], 2), round(ks[k]["min_us"], 2), round(ks[k]["max_us"], 2), b.get(k, ""),
                                     round(floor_us[k], 2) if k in floor_us else "", out["share_of_ceiling"].get(k, "")])
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
