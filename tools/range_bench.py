#!/usr/bin/env python3
"""usage: tools/range_bench.py [--reps 5] [--warmup 1] [--out profiles/range_bench.json] [--steps unlimited,limited,ao] [--grid 2048] [--step-timeout 240]

Distance-limited rays and the occlusion bake on the dragon stand-in at --grid^3 (2048).  Every step runs in a child process of its own under `timeout`; the first step
that fails ends the run (nothing more is started on the GPU) and what was measured up to there is still written.
  unlimited  mvrt_trace_batch_range with tMax = MVRT_MAX_FLOAT against mvrt_trace_batch on the same rays, a primary-like set (a pinhole camera's pixel grid) and
             an incoherent one (random origins around the grid, random targets in it): the price of the per-lane kernel against the streaming one
  limited    the same rays with tMax at 8 and at 64 voxels (directions normalised): rays/s and mean descents
  ao         mvrt_svo_surface_ao at K = 16 and 64, radius 8 voxels, over the full face list: milliseconds and rays/s, beside mvrt_svo_surface_quads itself
Median of --reps calls after --warmup calls, host clock between device synchronisations."""
import argparse
import os
import sys

import numpy as np

import benchkit as bk

MAXF = np.float32(3.402823466e38)


def ray_sets(origin, dps, res, n_side=1024, seed=11):
    """normalised directions, so that t is a distance in the units of dps"""
    f32 = np.float32
    lo = np.asarray(origin, f32)
    ext = f32(dps) * f32(res)
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


def step_rays(mv, args, which):
    svo, origin, dps = bk.built(mv, "dragon", args.grid)
    dps = np.float32(dps)
    rows = []
    for name, (ro, rd) in ray_sets(origin, dps, args.grid).items():
        n = len(ro)
        dev = [mv.DeviceArray.from_host(np.ascontiguousarray(a)) for a in (ro[:, 0], ro[:, 1], ro[:, 2], rd[:, 0], rd[:, 1], rd[:, 2])]
        t, nm, vi, de = mv.DeviceArray(n, np.float32), mv.DeviceArray(n, np.int32), mv.DeviceArray(n, np.uint32), mv.DeviceArray(n, np.uint32)
        base = dict(scene="dragon", grid=args.grid, rays=name, n=n)
        ms, ts = bk.timed_async(mv, lambda: svo.intersect_device(n, *dev, None, t, nm, vi, de), args.reps, args.warmup)
        stream_t, stream_de = t.to_host(), de.to_host()
        if which == "unlimited":
            rows.append(dict(op="trace_batch", ms=ms, all_ms=ts, rays_per_s=n / (ms * 1e-3), mean_descents=float(stream_de.mean()), hits=int((stream_t != MAXF).sum()), **base))
        limits = {"unlimited": (("maxf", MAXF),), "limited": (("8 voxels", np.float32(8) * dps), ("64 voxels", np.float32(64) * dps))}[which]
        for label, lim in limits:
            dlim = mv.DeviceArray.from_host(np.full(n, lim, np.float32))
            ms, ts = bk.timed_async(mv, lambda: svo.intersect_range_device(n, *dev, None, dlim, t, nm, vi, de), args.reps, args.warmup)
            got_t, got_de = t.to_host(), de.to_host()
            want_t = np.where((stream_t != MAXF) & (stream_t <= lim), stream_t, MAXF)
            rows.append(dict(op="trace_batch_range", tMax=label, ms=ms, all_ms=ts, rays_per_s=n / (ms * 1e-3), mean_descents=float(got_de.mean()),
                             mean_descents_unlimited=float(stream_de.mean()), hits=int((got_t != MAXF).sum()), equal_to_filtered_trace_batch=bool(np.array_equal(got_t, want_t)), **base))
            del dlim
    return rows


def step_ao(mv, args):
    svo, origin, dps = bk.built(mv, "dragon", args.grid)
    dps = np.float32(dps)
    n = svo.surface_quads_device()
    fv, fd = mv.DeviceArray(n, np.uint32), mv.DeviceArray(n, np.uint8)
    base = dict(scene="dragon", grid=args.grid, voxels=int(svo.info().numberOfVoxels), nFaces=n)
    ms, ts = bk.timed_async(mv, lambda: svo.surface_quads_device(n, fv, fd, None), args.reps, args.warmup)
    rows = [dict(op="surface_quads", ms=ms, all_ms=ts, **base)]
    op = mv.DeviceArray(n, np.uint16)
    for K in (16, 64):
        ms, ts = bk.timed_async(mv, lambda: svo.surface_ao_device(n, fv, fd, K, np.float32(8) * dps, op), args.reps, args.warmup)
        rows.append(dict(op="surface_ao", samples=K, radius_voxels=8, ms=ms, all_ms=ts, rays_per_s=n * K / (ms * 1e-3), mean_open_fraction=float(op.to_host().mean() / K), **base))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=2048)
    ap.add_argument("--steps", default="unlimited,limited,ao")
    bk.add_step_args(ap, reps=5, warmup=1, step_timeout=240, out=os.path.join(bk.ROOT, "profiles", "range_bench.json"))
    args = ap.parse_args()
    if args.step:
        import massivevoxelraytracing_amd as mv
        mv.set_device(0)
        for row in step_ao(mv, args) if args.step == "ao" else step_rays(mv, args, args.step):
            bk.emit(row)
        return 0
    return bk.run_steps(__file__, args.steps.split(","), lambda s: bk.flags(args, "reps", "warmup", "grid"), args.step_timeout, args.out, echo=bk.brief)[1]


if __name__ == "__main__":
    sys.exit(main())
