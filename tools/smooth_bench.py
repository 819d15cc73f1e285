#!/usr/bin/env python3
"""usage: tools/smooth_bench.py [--scenes dragon[:grid],tunnel[:grid]] [--reps 10] [--warmup 2] [--step-timeout 600] [--out profiles/smooth_bench.json]
                                [--no-host-route]

Cost of mvrt_svo_surface_smooth next to the mesh it smooths, on the procedural stand-ins (dragon 2048^3, tunnel 4096^3), every output into device arrays:
  mesh        mvrt_svo_surface_mesh
  smooth0     mvrt_svo_surface_smooth without an iteration, taking turns with mesh in one loop: the difference (table_ms) is the neighbour table, the two
              displacement buffers and the output kernel
  smooth4, smooth16   4 and 16 iterations of the plain weights, limit 127, taking turns in one loop
  iteration   no clock of its own: ( smooth16 - smooth4 ) / 12 as ms_per_iteration, from the fastest call of each; the algorithmic bytes of one iteration -- per vertex its own 8 bytes, 8
              per neighbour, the six 4-byte table words and one 8-byte store -- and the GB/s the two give; the clamped count of smooth4; peak_bytes = the most
              device memory the library held during one smooth4 call beyond the octree (mvrt_test_peak_bytes)
  host_route  once, on the first scene: the route a caller has without this call -- the mesh to the host, the same relaxation in numpy (corners recovered from
              the positions, a neighbour table from the indices, 4 iterations), the vertices back to the device; equal_to_gpu says the displacements agree
The two differences (table_ms, ms_per_iteration) are taken between the FASTEST calls, not between the medians: every call allocates gigabytes of scratch, and on
some runs the calls of a loop fall into two populations seconds apart; a median can land in either, and the slow population is a cost of
the allocations, not of the table or of an iteration.  The rows themselves carry the median and every call's time.
Median of --reps calls after --warmup calls; host clock around each call (every call blocks until its counts are back).  Output arrays are allocated before the
clock starts.  Every step runs in a child process of its own under --step-timeout seconds; a step that fails, is killed or runs out of time ends the run:
nothing more is started on the GPU behind it."""
import argparse
import ctypes
import sys
import time

import numpy as np

import benchkit as bk

SLOTS = np.array([(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)], np.int64)


def host_relax(corners, indices, iterations, weights, limit):
    """the rule of mvrt.h in numpy -> displacements (m, 3) int64"""
    m = len(corners)
    nbr = np.full((m, 6), -1, np.int64)
    idx = indices.astype(np.int64)
    for k in range(4):
        for step in (1, 3):
            a, b = idx[:, k], idx[:, (k + step) & 3]
            u = corners[b] - corners[a]
            nbr[a, np.argmax(np.abs(u), 1) * 2 + (u.sum(1) > 0)] = b
    has = nbr >= 0
    n = has.sum(1).astype(np.int64)[:, None]
    unit = (has[:, :, None] * SLOTS[None, :, :]).sum(1)
    d = np.zeros((m, 3), np.int64)
    for k in range(iterations):
        total = np.zeros((m, 3), np.int64)
        for s in range(6):
            total += np.where(has[:, s, None], d[np.maximum(nbr[:, s], 0)], 0)
        a = weights[k & 1] * (256 * unit + total - n * d)
        d = np.clip(d + np.sign(a) * ((2 * np.abs(a) + 256 * n) // (512 * n)), -limit, limit)
    return d


def step(args):
    """one child process: prints one JSON row per measurement"""
    import massivevoxelraytracing_amd as mv
    mv.set_device(0)
    name, res, op = args.step.split(":")
    res = int(res)
    svo, origin, dps = bk.built(mv, name, res)
    nf, nv = svo.surface_mesh_device()
    base = dict(scene=name, grid=res, voxels=svo.info().numberOfVoxels, nFaces=nf, nVertices=nv)
    fv, fd, idx, vtx = mv.DeviceArray(nf, np.uint32), mv.DeviceArray(nf, np.uint8), mv.DeviceArray((nf, 4), np.uint32), mv.DeviceArray((nv, 3), np.float32)
    disp, nbr = mv.DeviceArray((nv, 3), np.int32), mv.DeviceArray(nv, np.uint8)

    def params(k):
        p = mv.SmoothParams()
        mv._check(mv.lib().mvrt_smooth_default_params(ctypes.byref(p)))
        p.iterations = k
        return p

    def smooth(k):
        p = params(k)
        return lambda: svo.surface_smooth_device(p, nf, nv, fv, fd, idx, vtx, disp, nbr)

    if op == "mesh":
        (mesh_ms, mesh_ts), (s0_ms, s0_ts) = bk.timed_each(mv, [lambda: svo.surface_mesh_device(nf, nv, fv, fd, idx, vtx), smooth(0)], args.reps, args.warmup)
        bk.emit(base, op="mesh", ms=mesh_ms, all_ms=mesh_ts)
        bk.emit(base, op="smooth0", ms=s0_ms, all_ms=s0_ts, table_ms=min(s0_ts) - min(mesh_ts))  # (the fastest calls: see the head of this file)
    elif op == "iterate":
        last = {}
        (s4_ms, s4_ts), (s16_ms, s16_ts) = bk.timed_each(mv, [smooth(4), smooth(16)], args.reps, args.warmup, after=lambda j, result: last.__setitem__(j, result))
        bk.emit(base, op="smooth4", ms=s4_ms, all_ms=s4_ts, clamped=last[0][2])
        bk.emit(base, op="smooth16", ms=s16_ms, all_ms=s16_ts, clamped=last[1][2])
        peak = bk.peak_of(mv, smooth(4))
        degree_sum = int(np.unpackbits(nbr.to_host()).sum())
        per_iteration = (min(s16_ts) - min(s4_ts)) / 12.0  # (the fastest calls, like table_ms)
        nbytes = nv * (8 + 24 + 8) + 8 * degree_sum
        bk.emit(base, op="iteration", ms_per_iteration=per_iteration, bytes_per_iteration=nbytes, bytes_per_vertex=nbytes / max(nv, 1),
                gb_per_s=nbytes / (per_iteration * 1e6) if per_iteration > 0 else None, clamped=last[0][2], peak_bytes=peak)
    else:
        lower = np.asarray(origin, np.float32)
        svo.surface_smooth_device(params(4), nf, nv, fv, fd, idx, vtx, disp, nbr)
        want = disp.to_host()
        mv.synchronize()
        t0 = time.perf_counter()
        svo.surface_mesh_device(nf, nv, fv, fd, idx, vtx)
        v, i = vtx.to_host(), idx.to_host()
        t1 = time.perf_counter()
        corners = np.rint((v.astype(np.float64) - lower.astype(np.float64)) / np.float64(dps)).astype(np.int64)
        d = host_relax(corners, i, 4, (256, 256), 127)
        q = (256 * corners + d).astype(np.int32)
        out = (lower + ((q.astype(np.float32) * np.float32(0.00390625)) * np.float32(dps)).astype(np.float32)).astype(np.float32)
        t2 = time.perf_counter()
        back = mv.DeviceArray.from_host(out)
        mv.synchronize()
        t3 = time.perf_counter()
        bk.emit(base, op="host_route", ms=(t3 - t0) * 1e3, all_ms=[(t3 - t0) * 1e3], download_ms=(t1 - t0) * 1e3, numpy_ms=(t2 - t1) * 1e3, upload_ms=(t3 - t2) * 1e3,
                equal_to_gpu=bool(np.array_equal(d, want)))
        back.free()


def line(r):
    what = "%9.2f ms  (%.2f .. %.2f)" % (r["ms"], min(r["all_ms"]), max(r["all_ms"])) if "ms" in r else (
        "%.3f ms / iteration, %.1f B / vertex, %s GB/s, peak %s B" % (r["ms_per_iteration"], r["bytes_per_vertex"], r["gb_per_s"] and round(r["gb_per_s"], 1), r["peak_bytes"])
        if "ms_per_iteration" in r else r.get("skipped") or r.get("failed"))
    return "%-7s %5s %-10s %11s faces %11s vertices  %s" % (r.get("scene", r.get("step")), r.get("grid", ""), r.get("op", ""), r.get("nFaces", ""), r.get("nVertices", ""), what)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=bk.parse_scenes, default="dragon,tunnel")
    ap.add_argument("--no-host-route", action="store_true")
    bk.add_step_args(ap, reps=10, warmup=2, step_timeout=600)
    args = ap.parse_args()
    if args.step:
        return step(args)
    steps = ["%s:%d:%s" % (*scene, op) for scene in args.scenes for op in ("mesh", "iterate")]
    if not args.no_host_route:
        steps.append("%s:%d:host" % args.scenes[0])
    rows, rc = bk.run_steps(__file__, steps, lambda s: bk.flags(args, "reps", "warmup"), args.step_timeout, args.out, echo=bk.brief)
    bk.print_table(rows, line)
    return rc


if __name__ == "__main__":
    sys.exit(main())
