#!/usr/bin/env python3
"""Cost of steps under a sample mask (mvrt_pt_set_sample_mask) and of the two calls of adaptive sampling on the headline workload: bench.py's default scene
(dragon stand-in 2048^3), 1920x1080, frames of 4 steps.

Run on the GPU box under a time limit of its own, chained so that nothing starts after a failure:

    timeout -k 10 540 python3 tools/adaptive_bench.py --out profiles/adaptive_bench.json && ...

In ONE process, after a warm-up, the configurations are ALTERNATED --reps times; each measurement is --frames frames (clear, set the mask, device synchronise;
then TIMED: 4 steps, join, device synchronise), in ms per step of the host clock.  clearFrameBuffer drops the mask, so every frame sets it again; that call is
outside the timed region and measured on its own below, like mvrt_pt_error_mask.  The rays traced per step are recorded beside the times (mvrt_pt_stats): the
cost of a step follows its rays, not its pixels.  Configurations: no mask (measured twice per round: its spread over all its measurements is the run-to-run yardstick), an all-ones mask, seeded random masks
and block-coherent masks (a centred rectangle) of 1/2, 1/4 and 1/16 of the pixels.  Then one mvrt_pt_error_mask call and one mvrt_pt_set_sample_mask call (1/4
random mask), each timed over --calls calls.  The three acceptance statements are evaluated and written beside the figures; a fractional mask is also recorded
against fraction x the unmasked time."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="dragon")
    ap.add_argument("--grid-res", type=int, default=2048)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frame-steps", type=int, default=4)
    ap.add_argument("--frames", type=int, default=4, help="timed frames per measurement")
    ap.add_argument("--reps", type=int, default=5, help="rounds; every configuration is measured once per round, no mask twice")
    ap.add_argument("--calls", type=int, default=20, help="timed calls of error_mask / set_sample_mask")
    ap.add_argument("--detail", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import massivevoxelraytracing_amd as mv
    from massivevoxelraytracing_amd import scenes
    mv.lib()
    mv.set_device(0)
    verts, cols, emis = scenes.SCENES[args.scene](args.detail)
    origin, dps = scenes.bounding_grid(verts, args.grid_res)
    W, H = args.width, args.height
    n = W * H
    pt = mv.PathTracer()
    pt.setup(None)
    pt.set_moments(True)  # what error_mask reads; on in every configuration
    pt.resizeFrameBufferIfNeeded(None, W, H)
    hdr = os.path.join(ROOT, "tests", "golden", "monks_forest_s.hdr")
    pt.loadHDRI(None, hdr, hdr)
    pt.updateScene(verts, cols, emis, None, origin, dps, args.grid_res)
    info = pt.m_intersectorOctreeGPU.info()
    lo, hi = np.array(info.lower[:]), np.array(info.upper[:])
    centre = (lo + hi) / 2
    eye = centre + np.array([2.6, 1.5, 3.1])  # bench.py's dragon camera
    cam = scenes.look_at_camera(eye, centre, 40.0, float(np.linalg.norm(eye - centre)), 0.02)
    owned = pt.owned_pixels()

    def device_mask(m):
        host = np.zeros(owned, np.uint8)
        host[:n] = m.reshape(-1)
        return mv.DeviceArray.from_host(host)

    def rectangle(fraction):  # centred, the frame's aspect
        s = fraction ** 0.5
        w, h = int(round(W * s)), int(round(H * s))
        m = np.zeros((H, W), bool)
        m[(H - h) // 2:(H - h) // 2 + h, (W - w) // 2:(W - w) // 2 + w] = True
        return m

    rng = np.random.default_rng(2024)
    configs = [("no_mask", None, 1.0), ("all_ones", np.ones(n, bool), 1.0)]
    for f in (2, 4, 16):
        configs.append(("random_1/%d" % f, rng.random(n) < 1.0 / f, 1.0 / f))
    for f in (2, 4, 16):
        configs.append(("rectangle_1/%d" % f, rectangle(1.0 / f), 1.0 / f))
    masks = {name: (None if m is None else device_mask(m)) for name, m, _ in configs}
    active = {name: (n if m is None else int(m.sum())) for name, m, _ in configs}

    def frames(k, mask):
        """-> seconds spent in the steps of k frames"""
        spent = 0.0
        for _ in range(k):
            pt.clearFrameBuffer(None)
            if mask is not None:
                pt.set_sample_mask(mask)
            mv.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.frame_steps):
                pt.step(None, cam)
            pt.join(None)
            mv.synchronize()
            spent += time.perf_counter() - t0
        return spent

    def measure(name):
        frames(1, masks[name])  # warm-up of this configuration
        return frames(args.frames, masks[name]) * 1e3 / (args.frames * args.frame_steps)

    frames(3, None)
    rays = {}
    for name, _, _ in configs:  # rays (bounce, shadow and extra rays together) per step of each configuration, outside the timing
        pt.reset_stats()
        frames(1, masks[name])
        rays[name] = pt.stats()["rays"] / args.frame_steps
    times = {name: [] for name, _, _ in configs}
    for _ in range(args.reps):
        for name, _, _ in configs:
            times[name].append(measure(name))
        times["no_mask"].append(measure("no_mask"))

    # the two calls, on a frame with 64 samples per pixel
    frames(1, None)
    out_dev = mv.DeviceArray(owned, np.uint8)
    pt.error_mask(0.05, out_dev=out_dev)
    mv.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.calls):
        _, marked = pt.error_mask(0.05, out_dev=out_dev)
    error_ms = (time.perf_counter() - t0) * 1e3 / args.calls
    quarter = masks["random_1/4"]
    pt.set_sample_mask(quarter)
    t0 = time.perf_counter()
    for _ in range(args.calls):
        pt.set_sample_mask(quarter)
    set_ms = (time.perf_counter() - t0) * 1e3 / args.calls
    pt.set_sample_mask(None)

    base = times["no_mask"]
    med = statistics.median(base)
    spread = max(base) - min(base)
    rows = {}
    for name, _, fraction in configs:
        t = times[name]
        m = statistics.median(t)
        rows[name] = {"active_pixels": active[name], "fraction": round(active[name] / n, 5), "ms_per_step": [round(x, 4) for x in t], "median": round(m, 4),
                      "spread": round(max(t) - min(t), 4), "fraction_x_unmasked": round(active[name] / n * med, 4), "over_fraction_x_unmasked": round(m / (active[name] / n * med), 3),
                      "rays_per_step": int(rays[name]), "ray_share": round(rays[name] / rays["no_mask"], 5), "over_ray_share_x_unmasked": round(m / (rays[name] / rays["no_mask"] * med), 3)}
    small = [name for name, _, f in configs if f <= 0.25]
    from massivevoxelraytracing_amd import build as B
    out = {
        "library_source_digest": B.source_digest(),
        "workload": "%s stand-in %d^3, %dx%d, moments on, frames of %d steps (clear, set_sample_mask, sync; timed: steps, join, sync), %d timed frames per measurement, %d rounds alternated in one process" % (
            args.scene, args.grid_res, W, H, args.frame_steps, args.frames, args.reps),
        "device": mv.device_name(),
        "no_mask": {"median": round(med, 4), "spread": round(spread, 4), "measurements": len(base)},
        "configurations": rows,
        "error_mask_ms_per_call": round(error_ms, 4), "error_mask_marked_at_0.05_after_64spp": int(marked),
        "set_sample_mask_ms_per_call": round(set_ms, 4),
        "acceptance": {
            "1_all_ones_within_spread_of_no_mask": bool(abs(rows["all_ones"]["median"] - med) <= spread),
            "3_quarter_or_less_faster_by_more_than_spread": {name: bool(med - rows[name]["median"] > spread) for name in small},
        },
    }
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
