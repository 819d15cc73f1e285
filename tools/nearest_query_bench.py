#!/usr/bin/env python3
"""usage: tools/nearest_query_bench.py [--scenes dragon:2048,tunnel:4096] [--ops shift,closed,random,band,noseed] [--reps 5] [--warmup 1] [--queries 16777216]
                                      [--step-timeout 420] [--variant build/ab/libmvrt_exp.so] [--out profiles/nearest_query_bench.json]

Cost of the nearest-voxel query (mvrt_svo_nearest_voxels / mvrt_svo_nearest_between / mvrt_svo_transfer_attributes) on the procedural stand-ins:
  shift    nearest_between( a, a shifted by 8 cells ), listing and summary call
  closed   nearest_between( a, close_ball( a, 16 ) ) and back, then transfer_attributes of the closed set from the original (the closed set is painted a flat
           grey before every timed call, outside the clock: the ball closing itself colours its new cells by their nearest voxel), next to the host route the parent commit offers for it: read_voxels to the host + edit_voxels from
           the host.  The search of that route is not timed: the parent has none
  random   --queries uniformly random in-grid points through nearest_voxels: the unfriendly case
  band     the yardstick: distance_cells( 64 ), reach 8, the only device route of the parent commit to a nearest voxel outside the set
  noseed   the figures of shift and random once more without the seed: a library built by tools/build_variant.sh (--variant) with MVRT_NEAREST_QUERY_SEED=0.
           Skipped with a row that says so where that library is not there
Every call is reported (all_ms), with its median; host clock around each call (every call blocks); output arrays are allocated before the clock starts.  Per new
call also the peak scratch (mvrt_test_peak_bytes around one call) and the figures of mvrt_test_nearest_query_stats: visits per query, mean and most, and the voxels
compared; the peak is taken around the warm-up call.  A call the library refuses is reported with the library's message, never guessed.  Every step runs in a child process of its own under
`timeout -k 10 --step-timeout`; a step that fails, is killed or runs out of time ends the run: nothing more is started on the GPU behind it.  A child sizes no
thread pool of its own."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(mv, fn, reps, warmup, before=None):
    ts = []
    for i in range(warmup + reps):
        if before:
            before()
        mv.synchronize()
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), ts


def built(mv, name, res):
    from massivevoxelraytracing_amd import scenes
    verts, cols, emis = scenes.SCENES[name](1.0)
    origin, dps = scenes.bounding_grid(verts, res)
    svo = mv.IntersectorOctreeGPU()
    svo.build(verts, cols, emis, None, origin, dps, res)
    return svo, origin, dps


def peak_of(mv, fn):
    """the most bytes the library held during fn beyond what it held before"""
    held = mv.allocation_state()[1]
    mv.peak_bytes(reset=True)
    fn()
    return mv.peak_bytes() - held


def query_figures(mv):
    s = mv.nearest_query_stats()
    q = max(1, s["queries"])
    return dict(queries=s["queries"], visits_per_query=s["visits"] / q, most_visits=s["most"], compared_per_query=s["compared"] / q)


def step(args):
    """one child process: prints one JSON row per measurement"""
    import massivevoxelraytracing_amd as mv
    mv.set_device(0)
    name, res, op = args.step.split(":")
    res = int(res)
    a, origin, dps = built(mv, name, res)
    n = a.info().numberOfVoxels
    seed = os.environ.get("MVRT_NEAREST_QUERY_SEED", "1") != "0"
    base = dict(scene=name, grid=res, voxels=n, seed=seed)

    def emit(**kw):
        print(json.dumps(dict(kw, **base)), flush=True)

    def measure(label, fn, before=None, figures=True, reps=None, **extra):
        try:
            peak = peak_of(mv, (lambda: (before(), fn())) if before else fn)  # the warm-up call
            ms, ts = timed(mv, fn, args.reps if reps is None else reps, max(0, args.warmup - 1), before)
        except mv.MvrtError as e:
            emit(op=label, refused=str(e), **extra)
            return None
        emit(op=label, ms=ms, all_ms=ts, peak_bytes=peak, peak_includes_reset=bool(before), **dict(query_figures(mv) if figures else {}, **extra))
        return ms

    def random_queries():
        q = np.random.default_rng(7).integers(0, res, size=(args.queries, 3), dtype=np.int32)
        return mv.DeviceArray.from_host(q)

    if op == "shift":
        d2, near = mv.DeviceArray(n, np.uint64), mv.DeviceArray(n, np.uint32)
        r = {}
        measure("between_shift8", lambda: r.update(a.nearest_between_device(a, (8, 0, 0), capacity=n, dist2=d2, nearest=near)))
        measure("between_shift8_summary", lambda: r.update(a.nearest_between_device(a, (8, 0, 0))))
        emit(op="between_shift8_result", **r)
    elif op == "closed":
        c = mv.IntersectorOctreeGPU()
        xyz, attrs = mv.DeviceArray((n, 3), np.uint32), mv.DeviceArray((n, 8), np.uint8)
        mv._check(mv.lib().mvrt_svo_read_voxels(a._h, xyz.ptr, attrs.ptr, None))
        c.build_voxels(xyz, attrs, origin=origin, dps=dps, gridRes=res)
        added = c.close_ball(16)
        m = c.info().numberOfVoxels
        emit(op="close_ball16", added=added, voxels_closed=m)
        d2, near = mv.DeviceArray(max(n, m), np.uint64), mv.DeviceArray(max(n, m), np.uint32)
        r = {}
        measure("between_a_to_closed", lambda: r.update(a.nearest_between_device(c, capacity=n, dist2=d2, nearest=near)))
        emit(op="between_a_to_closed_result", **r)
        measure("between_closed_to_a", lambda: r.update(c.nearest_between_device(a, capacity=m, dist2=d2, nearest=near)))
        emit(op="between_closed_to_a_result", **r)
        cx, ca = mv.DeviceArray((m, 3), np.uint32), mv.DeviceArray((m, 8), np.uint8)
        mv._check(mv.lib().mvrt_svo_read_voxels(c._h, cx.ptr, ca.ptr, None))
        # (the ball closing already gives a new cell the bytes of its nearest voxel: with the closed set's own bytes the transfer would find nothing to change.
        # The clean geometry of the use case has no colours yet: a flat grey)
        grey = mv.DeviceArray.from_host(np.tile(np.array([128, 128, 128, 255, 0, 0, 0, 255], np.uint8), (m, 1)))
        reset = lambda: c.edit_voxels(cx, grey)
        out = []
        measure("transfer_closed_from_a", lambda: out.append(c.transfer_attributes(a)), before=reset)
        emit(op="transfer_closed_from_a_result", changed=out[-1][0], beyond=out[-1][1])
        host = {}

        def host_route():  # what the parent commit offers: the voxels to the host and the new bytes back (the search between the two is not timed: there is none)
            host["xyz"], host["at"] = c.read_voxels()
            c.edit_voxels(host["xyz"], host["at"])
        measure("host_route_read_plus_edit", host_route, before=reset, figures=False)
    elif op == "random":
        q = random_queries()
        d2, near, at = mv.DeviceArray(args.queries, np.uint64), mv.DeviceArray(args.queries, np.uint32), mv.DeviceArray((args.queries, 8), np.uint8)
        ms = measure("nearest_voxels_random", lambda: a.nearest_voxels_device(args.queries, q, dist2=d2, nearest=near, attribs=at))
        if ms:
            emit(op="nearest_voxels_random_rate", queries_per_s=args.queries / (ms * 1e-3))
    elif op == "band":
        measure("yardstick_distance_cells_64_count", lambda: a.distance_cells_device(64), figures=False, radius2=64)
    elif op == "noseed":  # one call each: the figures are what is wanted
        a.nearest_between_device(a, (8, 0, 0))
        emit(op="between_shift8_summary_figures", **query_figures(mv))
        q = random_queries()
        a.nearest_voxels_device(args.queries, q)
        emit(op="nearest_voxels_random_figures", **query_figures(mv))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="dragon:2048,tunnel:4096")
    ap.add_argument("--ops", default="shift,closed,random,band,noseed")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--queries", type=int, default=1 << 24)
    ap.add_argument("--step-timeout", type=int, default=420)
    ap.add_argument("--variant", default=os.path.join(ROOT, "build", "ab", "libmvrt_exp.so"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        return step(args)
    steps = [s + ":" + op for s in args.scenes.split(",") for op in args.ops.split(",")]
    rows, rc = [], 0

    def save():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(rows, f, indent=1)

    for s in steps:
        env = dict(os.environ)
        if s.endswith(":noseed"):
            if not os.path.exists(args.variant):
                rows.append(dict(step=s, skipped="no experiment build at %s (tools/build_variant.sh exp)" % os.path.relpath(args.variant, ROOT)))
                continue
            env.update(MVRT_LIB=args.variant, MVRT_NEAREST_QUERY_SEED="0")
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", s, "--reps", str(args.reps), "--warmup", str(args.warmup),
               "--queries", str(args.queries)]
        print("step", s, flush=True)
        out = subprocess.run(cmd, stdout=subprocess.PIPE, env=env)
        for line in out.stdout.decode().splitlines():
            if line.startswith("{"):
                rows.append(json.loads(line))
                print(line, flush=True)
        if out.returncode != 0:
            rows.append(dict(step=s, failed="no result within %d s" % args.step_timeout if out.returncode in (124, 137) else "exit status %d" % out.returncode))
            rc = 1
            break  # nothing more is started on the GPU behind a step that failed
        save()  # (kept up to date step by step)
    save()
    for r in rows:
        what = "%9.2f ms" % r["ms"] if "ms" in r else r.get("refused") or r.get("skipped") or r.get("failed") or ""
        print("%-7s %5s %-36s seed %-5s %10s voxels  %s  %s" % (r.get("scene", r.get("step")), r.get("grid", ""), r.get("op", ""), r.get("seed", ""), r.get("voxels", ""), what,
                                                               "visits/query %.1f most %d" % (r["visits_per_query"], r["most_visits"]) if "visits_per_query" in r else ""), file=sys.stderr)
    return rc


if __name__ == "__main__":
    sys.exit(main())
