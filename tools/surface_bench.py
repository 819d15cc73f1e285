#!/usr/bin/env python3
"""usage: tools/surface_bench.py [--scenes dragon[:grid],tunnel[:grid]] [--reps 10] [--warmup 2] [--out profiles/surface_bench.json] [--no-host-method]

Cost of extracting the voxel surface on the procedural stand-ins (dragon 2048^3, tunnel 4096^3):
  masks   mvrt_svo_surface_masks into a device array (16 B read + 1 B written per voxel)
  quads   mvrt_svo_surface_quads into device arrays (masks + scan + 53 B written per face)
  mesh    mvrt_svo_surface_mesh into device arrays (masks + scan + corner keys + radix sort + ranks)
  merged  mvrt_svo_surface_merged into device arrays, once per flag combination (per direction: keys + radix sort + heads, twice; with the weld flag the
          corner sort as in mesh): nRects, nRects / nFaces and the time
Median of --reps calls after --warmup calls; host clock around each call (every call blocks until its counts are back).  Output arrays are allocated
before the clock starts.  The achieved bytes per second of the whole masks and quads CALLS stand next to the 8 TB/s HBM peak; kernel times come from a
kernel trace of its own (rocprofv3 --kernel-trace --stats -- python tools/surface_bench.py --reps 3 --no-host-method).
Once, on the dragon: the only route without this feature -- mvrt_svo_read_voxels + the reference's host method (voxMesh.cpp:138-148: six searches per
voxel in the sorted codes), here with numpy searchsorted on all cores numpy uses, masks only."""
import argparse
import json
import sys
import time

import numpy as np

import benchkit as bk
import massivevoxelraytracing_amd as mv

HBM_PEAK = 8.0e12
DIRS = ((1, -1), (1, +1), (2, -1), (0, +1), (2, +1), (0, -1))


def morton(xyz):
    m = np.zeros(len(xyz), np.uint64)
    for b in range(21):
        for axis in range(3):
            m |= ((xyz[:, axis].astype(np.uint64) >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + axis)
    return m


def host_method(svo, res):
    """read_voxels + six searches per voxel in the sorted codes -> (masks, seconds)"""
    t0 = time.perf_counter()
    xyz, _ = svo.read_voxels()
    codes = morton(xyz)
    out = np.zeros(len(xyz), np.uint8)
    for d, (axis, step) in enumerate(DIRS):
        p = xyz.astype(np.int64)
        p[:, axis] += step
        inside = (p[:, axis] >= 0) & (p[:, axis] < res)
        want = morton(p[inside])
        at = np.minimum(np.searchsorted(codes, want), len(codes) - 1)
        present = np.zeros(len(xyz), bool)
        present[inside] = codes[at] == want
        out |= (~present).astype(np.uint8) << d
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=bk.parse_scenes, default="dragon,tunnel")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host-method", action="store_true")
    args = ap.parse_args()
    mv.set_device(0)
    rows = []

    def emit(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    def clock(fn):  # warm-ups first, then synchronize() and the clock around each blocking call
        return bk.timed(mv, fn, args.reps, args.warmup, warmup_first=True)

    for name, res in args.scenes:
        svo, _, _ = bk.built(mv, name, res)
        n_vox = svo.info().numberOfVoxels
        n_faces, n_vertices = svo.surface_mesh_device()
        base = dict(scene=name, grid=res, voxels=n_vox, nFaces=n_faces, nVertices=n_vertices)
        masks = mv.DeviceArray(n_vox, np.uint8)
        ms, ts = clock(lambda: svo.surface_masks_device(masks))
        rate = n_vox * 17 / (ms * 1e-3)
        emit(op="masks", ms=ms, all_ms=ts, bytes=n_vox * 17, bytes_per_s=rate, of_hbm_peak=rate / HBM_PEAK, **base)
        fv, fd = mv.DeviceArray(n_faces, np.uint32), mv.DeviceArray(n_faces, np.uint8)
        pos = mv.DeviceArray((n_faces, 12), np.float32)
        ms, ts = clock(lambda: svo.surface_quads_device(n_faces, fv, fd, pos))
        rate = n_faces * 53 / (ms * 1e-3)
        emit(op="quads", ms=ms, all_ms=ts, bytes=n_faces * 53, bytes_per_s=rate, of_hbm_peak=rate / HBM_PEAK, **base)
        del pos
        idx, vtx = mv.DeviceArray((n_faces, 4), np.uint32), mv.DeviceArray((n_vertices, 3), np.float32)
        ms, ts = clock(lambda: svo.surface_mesh_device(n_faces, n_vertices, fv, fd, idx, vtx))
        emit(op="mesh", ms=ms, all_ms=ts, **base)
        del idx, vtx, fv, fd
        for flags in (0, mv.SURFACE_MERGE_ANY_ATTRIBUTE, mv.SURFACE_MERGE_WELD, mv.SURFACE_MERGE_ANY_ATTRIBUTE | mv.SURFACE_MERGE_WELD):
            weld = bool(flags & mv.SURFACE_MERGE_WELD)
            _, n_rects, n_welded = svo.surface_merged_device(flags)
            rv, rd, rs = mv.DeviceArray(n_rects, np.uint32), mv.DeviceArray(n_rects, np.uint8), mv.DeviceArray((n_rects, 2), np.uint32)
            pos = None if weld else mv.DeviceArray((n_rects, 12), np.float32)
            idx, vtx = (mv.DeviceArray((n_rects, 4), np.uint32), mv.DeviceArray((n_welded, 3), np.float32)) if weld else (None, None)
            ms, ts = clock(lambda: svo.surface_merged_device(flags, n_rects, n_welded, rv, rd, rs, pos, idx, vtx))
            emit(op="merged", flags=flags, any_attribute=bool(flags & mv.SURFACE_MERGE_ANY_ATTRIBUTE), weld=weld, nRects=n_rects, nMergedVertices=n_welded,
                 rects_per_face=n_rects / max(n_faces, 1), ms=ms, all_ms=ts, **base)
            del rv, rd, rs, pos, idx, vtx
        if name == "dragon" and not args.no_host_method:
            got, s = host_method(svo, res)
            emit(op="host_method_masks", ms=s * 1e3, equal_to_gpu=bool(np.array_equal(got, masks.to_host())), **base)
        del svo
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
    for r in rows:
        op = r["op"] + ("" if "flags" not in r else " flags %d: %d rects, %.4f per face" % (r["flags"], r["nRects"], r["rects_per_face"]))
        print("%-7s %5d %-18s %9d voxels %10d faces %9.2f ms" % (r["scene"], r["grid"], op, r["voxels"], r["nFaces"], r["ms"]), file=sys.stderr)


if __name__ == "__main__":
    main()
