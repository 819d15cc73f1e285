#!/usr/bin/env python3
"""usage: tools/range_bench.py [--reps 5] [--warmup 1] [--out profiles/range_bench.json] [--steps unlimited,limited,ao] [--step-timeout 240]

Distance-limited rays and the occlusion bake on the dragon 2048^3 stand-in.  Every step runs in a child process of its own under `timeout`; the first step
that fails ends the run (nothing more is started on the GPU) and what was measured up to there is still written.
  unlimited  mvrt_trace_batch_range with tMax = MVRT_MAX_FLOAT against mvrt_trace_batch on the same rays, a primary-like set (a pinhole camera's pixel grid) and
             an incoherent one (random origins around the grid, random targets in it): the price of the per-lane kernel against the streaming one
  limited    the same rays with tMax at 8 and at 64 voxels (directions normalised): rays/s and mean descents
  ao         mvrt_svo_surface_ao at K = 16 and 64, radius 8 voxels, over the full face list: milliseconds and rays/s, beside mvrt_svo_surface_quads itself
Median of --reps calls after --warmup calls, host clock between device synchronisations."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RES = 2048
MAXF = np.float32(3.402823466e38)


def timed(mv, fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        mv.synchronize()
        t0 = time.perf_counter()
        fn()
        mv.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), ts


def ray_sets(origin, dps, n_side=1024, seed=11):
    """normalised directions, so that t is a distance in the units of dps"""
    f32 = np.float32
    lo = np.asarray(origin, f32)
    ext = f32(dps) * f32(RES)
    c = lo + ext / 2
    eye = (c + np.array([0.9, 0.55, 1.3], f32) * ext).astype(f32)
    front = (c - eye) / np.linalg.norm(c - eye)
    right = np.cross(front, [0, 1, 0])
    right /= np.linalg.norm(right)
    up = np.cross(right, front)
    s = (np.arange(n_side, dtype=f32) + f32(0.5)) / f32(n_side) * 2 - 1
    a, b = np.meshgrid(s * f32(0.45), -s * f32(0.45))
    rd = front[None, :] + a.reshape(-1, 1) * right[None, :] + b.reshape(-1, 1) * up[None, :]
    primary = (np.ascontiguousarray(np.broadcast_to(eye, rd.shape), f32), rd)
    rng = np.random.default_rng(seed)
    n = n_side * n_side
    ro = (c + (rng.random((n, 3)) - 0.5) * ext * 2.5).astype(f32)
    tgt = (lo + rng.random((n, 3)) * ext).astype(f32)
    incoherent = (ro, tgt - ro)
    out = {}
    for name, (o, d) in (("primary", primary), ("incoherent", incoherent)):
        d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
        out[name] = (o.astype(f32), d)
    return out


def build_dragon(mv):
    from massivevoxelraytracing_amd import scenes
    verts, cols, emis = scenes.SCENES["dragon"](1.0)
    origin, dps = scenes.bounding_grid(verts, RES)
    svo = mv.IntersectorOctreeGPU()
    svo.build(verts, cols, emis, None, origin, dps, RES)
    return svo, origin, np.float32(dps)


def step_rays(mv, args, which):
    svo, origin, dps = build_dragon(mv)
    rows = []
    for name, (ro, rd) in ray_sets(origin, dps).items():
        n = len(ro)
        dev = [mv.DeviceArray.from_host(np.ascontiguousarray(a)) for a in (ro[:, 0], ro[:, 1], ro[:, 2], rd[:, 0], rd[:, 1], rd[:, 2])]
        t, nm, vi, de = mv.DeviceArray(n, np.float32), mv.DeviceArray(n, np.int32), mv.DeviceArray(n, np.uint32), mv.DeviceArray(n, np.uint32)
        base = dict(scene="dragon", grid=RES, rays=name, n=n)
        ms, ts = timed(mv, lambda: svo.intersect_device(n, *dev, None, t, nm, vi, de), args.reps, args.warmup)
        stream_t, stream_de = t.to_host(), de.to_host()
        if which == "unlimited":
            rows.append(dict(op="trace_batch", ms=ms, all_ms=ts, rays_per_s=n / (ms * 1e-3), mean_descents=float(stream_de.mean()), hits=int((stream_t != MAXF).sum()), **base))
        limits = {"unlimited": (("maxf", MAXF),), "limited": (("8 voxels", np.float32(8) * dps), ("64 voxels", np.float32(64) * dps))}[which]
        for label, lim in limits:
            dlim = mv.DeviceArray.from_host(np.full(n, lim, np.float32))
            ms, ts = timed(mv, lambda: svo.intersect_range_device(n, *dev, None, dlim, t, nm, vi, de), args.reps, args.warmup)
            got_t, got_de = t.to_host(), de.to_host()
            want_t = np.where((stream_t != MAXF) & (stream_t <= lim), stream_t, MAXF)
            rows.append(dict(op="trace_batch_range", tMax=label, ms=ms, all_ms=ts, rays_per_s=n / (ms * 1e-3), mean_descents=float(got_de.mean()),
                             mean_descents_unlimited=float(stream_de.mean()), hits=int((got_t != MAXF).sum()), equal_to_filtered_trace_batch=bool(np.array_equal(got_t, want_t)), **base))
            del dlim
    return rows


def step_ao(mv, args):
    svo, origin, dps = build_dragon(mv)
    n = svo.surface_quads_device()
    fv, fd = mv.DeviceArray(n, np.uint32), mv.DeviceArray(n, np.uint8)
    base = dict(scene="dragon", grid=RES, voxels=int(svo.info().numberOfVoxels), nFaces=n)
    ms, ts = timed(mv, lambda: svo.surface_quads_device(n, fv, fd, None), args.reps, args.warmup)
    rows = [dict(op="surface_quads", ms=ms, all_ms=ts, **base)]
    op = mv.DeviceArray(n, np.uint16)
    for K in (16, 64):
        ms, ts = timed(mv, lambda: svo.surface_ao_device(n, fv, fd, K, np.float32(8) * dps, op), args.reps, args.warmup)
        rows.append(dict(op="surface_ao", samples=K, radius_voxels=8, ms=ms, all_ms=ts, rays_per_s=n * K / (ms * 1e-3), mean_open_fraction=float(op.to_host().mean() / K), **base))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_bench.json"))
    ap.add_argument("--steps", default="unlimited,limited,ao")
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        import massivevoxelraytracing_amd as mv
        mv.set_device(0)
        rows = step_ao(mv, args) if args.child == "ao" else step_rays(mv, args, args.child)
        print("ROWS " + json.dumps(rows), flush=True)
        return 0
    rows, status = [], 0
    for step in args.steps.split(","):
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--child", step, "--reps", str(args.reps), "--warmup", str(args.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        got = [json.loads(line[5:]) for line in r.stdout.splitlines() if line.startswith("ROWS ")]
        if r.returncode != 0 or not got:
            print("step %s failed with status %d; stopping here\n%s" % (step, r.returncode, r.stderr[-2000:]), file=sys.stderr)
            status = 1
            break
        for row in got[0]:
            rows.append(row)
            print(json.dumps({k: v for k, v in row.items() if k != "all_ms"}), flush=True)
    with open(args.out, "w") as f:
        json.dump(rows, f, indent=1)
    return status


if __name__ == "__main__":
    sys.exit(main())
