#!/usr/bin/env python3
"""usage: tools/resample_bench.py [--scenes dragon[:grid],tunnel[:grid]] [--cases identity,turn90,turn30,magnify2] [--reps 5] [--warmup 1] [--host-reps 1] [--step-timeout 420]
                                  [--out profiles/resample_bench.json]

Cost of the resampling calls on the procedural stand-ins (dragon 2048^3, tunnel 4096^3), per scene and case:
  identity   the set onto its own grid, cell for cell
  turn90     a quarter turn about z about the grid centre (a signed permutation, exact)
  turn30     30 degrees about (1, 2, 3) about the grid centre
  magnify2   the scene built at half the gridRes, onto the full grid at twice the size: every voxel a 2x2x2 block
and per case:
  resample_count / resample_list   mvrt_svo_resample_voxels, the sizing call and the listing of all three arrays into device arrays
  resample                         mvrt_svo_resample into a second handle; with the frontier sizes per level (mvrt_test_resample_stats) and peak_bytes, the most
                                   device memory the library held during one call beyond what it held before (mvrt_test_peak_bytes)
  host_route                       the same octree by the route that exists without the call: mvrt_svo_read_voxels to the host, the point rule in numpy int64 on
                                   the destination cells around the forward image of every voxel, the list back through mvrt_svo_build_voxels; `agrees` says that
                                   it left the same number of voxels
Median of --reps calls after --warmup calls (host_route: --host-reps calls, no warm-up: seconds each); host clock around each call (every call blocks).  A call the
library refuses is reported with its message, never guessed.  MVRT_LIB in the environment selects another build of the library.
Every step runs in a child process of its own under --step-timeout seconds; a step that fails, is killed or runs out of time ends the run: nothing more is
started on the GPU behind it."""
import argparse
import itertools
import os
import sys

import numpy as np

import benchkit as bk

CASES = ("identity", "turn90", "turn30", "magnify2")
F = 24


def rotation(axis, degrees):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    r = np.radians(degrees)
    return np.eye(3) + np.sin(r) * K + (1 - np.cos(r)) * (K @ K)


def transform(case, rs, rd):
    """the inverse map in cell units about the centres of the two grids -> (m (9,) int64, t (3,) int64)"""
    A = {"identity": np.eye(3), "turn90": rotation((0, 0, 1), -90.0), "turn30": rotation((1, 2, 3), -30.0), "magnify2": np.eye(3) * 0.5}[case]
    b = np.full(3, rs / 2.0) - A @ np.full(3, rd / 2.0)
    return np.rint(A.reshape(9) * 2.0 ** F).astype(np.int64), np.rint(b * 2.0 ** (F + 1)).astype(np.int64)


def host_route(src, dst, m, t, rd, origin, dps, chunk=1 << 21):
    """read the list, resample on the host, build: what a caller does without mvrt_svo_resample.  The map is invertible here: the destination cells whose centre
    can map into a voxel lie in the box of the voxel's forward image, a few per voxel; the point rule itself decides"""
    xs, at = src.read_voxels()
    rs = int(src.info().gridRes)
    M = m.reshape(3, 3)
    inv = np.linalg.inv(M / 2.0 ** F)
    b = t / 2.0 ** (F + 1)
    corners = np.array(list(itertools.product((0.0, 1.0), repeat=3))) @ inv.T
    lo_off, hi_off, eps = corners.min(0) - 0.5, corners.max(0) - 0.5, 1e-2  # (the fixed point moves a centre by less than 1e-3 cells on these grids)
    out_xyz, out_at = [], []
    for k in range(0, len(xs), chunk):
        s = xs[k:k + chunk].astype(np.int64)
        base = (s - b) @ inv.T
        c_lo, c_hi = np.ceil(base + lo_off - eps).astype(np.int64), np.floor(base + hi_off + eps).astype(np.int64)
        width = (c_hi - c_lo).max(0) + 1
        for off in itertools.product(*[range(int(w)) for w in width]):
            c = c_lo + np.array(off, np.int64)
            ok = ((c <= c_hi) & (c >= 0) & (c < rd)).all(1)
            cc = c[ok]
            hit = ((((2 * cc + 1) @ M.T + t) >> (F + 1)) == s[ok]).all(1)
            out_xyz.append(cc[hit].astype(np.uint32))
            out_at.append(at[k:k + chunk][ok][hit])
    xyz, attribs = np.concatenate(out_xyz), np.concatenate(out_at)
    attribs[:, [3, 7]] = 255
    assert (xs < rs).all()
    dst.build_voxels(xyz, attribs, origin=origin, dps=dps, gridRes=rd)
    return int(dst.info().numberOfVoxels)


def step(args):
    """one child process: prints one JSON row per measurement"""
    import massivevoxelraytracing_amd as mv
    mv.set_device(0)
    name, rd, case = args.step.split(":")
    rd = int(rd)
    rs = rd // 2 if case == "magnify2" else rd
    src, origin, dps = bk.built(mv, name, rs)
    dps = np.float32(dps * np.float32(rs / rd))  # the same box on the destination grid (exact: a power of two)
    m, t = transform(case, rs, rd)
    xf = mv.CellTransform.make(m, t)
    dst = mv.IntersectorOctreeGPU()
    base = dict(scene=name, case=case, src_grid=rs, grid=rd, voxels=src.info().numberOfVoxels, lib=os.path.basename(mv.LIB_PATH))

    def measure(label, fn, reps=args.reps, warmup=args.warmup):
        return bk.timed_or_refused(mv, base, label, fn, reps, warmup)

    n = measure("resample_count", lambda: src.resample_voxels_device(xf, rd))
    if n:
        xyz, at, so = mv.DeviceArray((n, 3), np.uint32), mv.DeviceArray((n, 8), np.uint8), mv.DeviceArray(n, np.uint32)
        measure("resample_list", lambda: src.resample_voxels_device(xf, rd, n, xyz, at, so))
        del xyz, at, so
    peaks = []

    def call():
        held = mv.allocation_state()[1]
        mv.peak_bytes(reset=True)
        src.resample(xf, dst, origin, dps, rd)
        peaks.append(mv.peak_bytes() - held)
        return int(dst.info().numberOfVoxels)

    got = measure("resample", call)
    if got is not None:
        bk.emit(base, op="resample_stats", frontier=mv.resample_stats()["frontier"], peak_bytes=int(max(peaks)), result=got)
    twin = mv.IntersectorOctreeGPU()
    host = measure("host_route", lambda: host_route(src, twin, m, t, rd, origin, dps), reps=args.host_reps, warmup=0)
    if host is not None and got is not None:
        bk.emit(base, op="host_route_check", agrees=bool(host == got), result=host)


def line(r):
    what = "%9.2f ms" % r["ms"] if "ms" in r else r.get("refused") or r.get("failed") or ""
    return "%-7s %5s %-9s %-16s %10s voxels  %s  -> %s %s" % (r.get("scene", r.get("step")), r.get("grid", ""), r.get("case", ""), r.get("op", ""), r.get("voxels", ""), what,
                                                              r.get("result", ""), r.get("frontier", ""))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=bk.parse_scenes, default="dragon,tunnel")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--host-reps", type=int, default=1)
    bk.add_step_args(ap, reps=5, warmup=1, step_timeout=420)
    args = ap.parse_args()
    if args.step:
        return step(args)
    steps = ["%s:%d:%s" % (name, res, c) for name, res in args.scenes for c in args.cases.split(",")]
    rows, rc = bk.run_steps(__file__, steps, lambda s: bk.flags(args, "reps", "warmup", "host_reps"), args.step_timeout, args.out)
    bk.print_table(rows, line)
    return rc


if __name__ == "__main__":
    sys.exit(main())
