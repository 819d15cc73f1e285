#!/usr/bin/env python3
"""usage: tools/resample_bench.py [--scenes dragon,tunnel] [--cases identity,turn90,turn30,magnify2] [--reps 5] [--warmup 1] [--host-reps 1] [--step-timeout 420]
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
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRID = {"dragon": 2048, "tunnel": 4096}
CASES = ("identity", "turn90", "turn30", "magnify2")
F = 24


def built(mv, name, res):
    from massivevoxelraytracing_amd import scenes
    verts, cols, emis = scenes.SCENES[name](1.0)
    origin, dps = scenes.bounding_grid(verts, res)
    svo = mv.IntersectorOctreeGPU()
    svo.build(verts, cols, emis, None, origin, dps, res)
    return svo, origin, dps


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
    name, case = args.step.split(":")
    rd = GRID[name]
    rs = rd // 2 if case == "magnify2" else rd
    src, origin, dps = built(mv, name, rs)
    dps = np.float32(dps * np.float32(rs / rd))  # the same box on the destination grid (exact: a power of two)
    m, t = transform(case, rs, rd)
    xf = mv.CellTransform.make(m, t)
    dst = mv.IntersectorOctreeGPU()
    base = dict(scene=name, case=case, src_grid=rs, grid=rd, voxels=src.info().numberOfVoxels, lib=os.path.basename(mv.LIB_PATH))

    def emit(**kw):
        print(json.dumps(dict(base, **kw)), flush=True)

    def timed(label, fn, reps=args.reps, warmup=args.warmup, **kw):
        ts, result = [], None
        for i in range(warmup + reps):
            mv.synchronize()
            t0 = time.perf_counter()
            try:
                result = fn()
            except mv.MvrtError as err:
                emit(op=label, refused=str(err), **kw)
                return None
            if i >= warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
        emit(op=label, ms=float(np.median(ts)), all_ms=ts, result=result, **kw)
        return result

    n = timed("resample_count", lambda: src.resample_voxels_device(xf, rd))
    if n:
        xyz, at, so = mv.DeviceArray((n, 3), np.uint32), mv.DeviceArray((n, 8), np.uint8), mv.DeviceArray(n, np.uint32)
        timed("resample_list", lambda: src.resample_voxels_device(xf, rd, n, xyz, at, so))
        del xyz, at, so
    peaks = []

    def call():
        held = mv.allocation_state()[1]
        mv.peak_bytes(reset=True)
        src.resample(xf, dst, origin, dps, rd)
        peaks.append(mv.peak_bytes() - held)
        return int(dst.info().numberOfVoxels)

    got = timed("resample", call)
    if got is not None:
        emit(op="resample_stats", frontier=mv.resample_stats()["frontier"], peak_bytes=int(max(peaks)), result=got)
    twin = mv.IntersectorOctreeGPU()
    host = timed("host_route", lambda: host_route(src, twin, m, t, rd, origin, dps), reps=args.host_reps, warmup=0)
    if host is not None and got is not None:
        emit(op="host_route_check", agrees=bool(host == got), result=host)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="dragon,tunnel")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--step-timeout", type=int, default=420)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        return step(args)
    steps = [":".join((s, c)) for s in args.scenes.split(",") for c in args.cases.split(",")]
    rows, rc = [], 0
    for s in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", s, "--reps", str(args.reps), "--warmup", str(args.warmup), "--host-reps", str(args.host_reps)]
        print("step", s, flush=True)
        try:
            out = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            rows.append(dict(step=s, failed="no result within %d s" % args.step_timeout))
            rc = 1
            break
        for line in out.stdout.decode().splitlines():
            if line.startswith("{"):
                rows.append(json.loads(line))
                print(line, flush=True)
        if out.returncode != 0:
            rows.append(dict(step=s, failed="exit status %d" % out.returncode))
            rc = 1
            break  # nothing more is started on the GPU behind a step that failed
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
    for r in rows:
        what = "%9.2f ms" % r["ms"] if "ms" in r else r.get("refused") or r.get("failed") or ""
        print("%-7s %5s %-9s %-16s %10s voxels  %s  -> %s %s" % (r.get("scene", r.get("step")), r.get("grid", ""), r.get("case", ""), r.get("op", ""), r.get("voxels", ""), what,
                                                                r.get("result", ""), r.get("frontier", "")), file=sys.stderr)
    return rc


if __name__ == "__main__":
    sys.exit(main())
