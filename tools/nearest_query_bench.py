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
import os
import sys

import numpy as np

import benchkit as bk


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
    a, origin, dps = bk.built(mv, name, res)
    n = a.info().numberOfVoxels
    seed = os.environ.get("MVRT_NEAREST_QUERY_SEED", "1") != "0"
    base = dict(scene=name, grid=res, voxels=n, seed=seed)

    def measure(label, fn, before=None, figures=True, reps=None, **extra):
        try:
            peak = bk.peak_of(mv, (lambda: (before(), fn())) if before else fn)  # the warm-up call
            ms, ts = bk.timed(mv, fn, args.reps if reps is None else reps, max(0, args.warmup - 1), before=before)
        except mv.MvrtError as e:
            bk.emit(base, op=label, refused=str(e), **extra)
            return None
        bk.emit(base, op=label, ms=ms, all_ms=ts, peak_bytes=peak, peak_includes_reset=bool(before), **dict(query_figures(mv) if figures else {}, **extra))
        return ms

    def random_queries():
        q = np.random.default_rng(7).integers(0, res, size=(args.queries, 3), dtype=np.int32)
        return mv.DeviceArray.from_host(q)

    if op == "shift":
        d2, near = mv.DeviceArray(n, np.uint64), mv.DeviceArray(n, np.uint32)
        r = {}
        measure("between_shift8", lambda: r.update(a.nearest_between_device(a, (8, 0, 0), capacity=n, dist2=d2, nearest=near)))
        measure("between_shift8_summary", lambda: r.update(a.nearest_between_device(a, (8, 0, 0))))
        bk.emit(base, op="between_shift8_result", **r)
    elif op == "closed":
        c = mv.IntersectorOctreeGPU()
        xyz, attrs = bk.snapshot(mv, a)
        c.build_voxels(xyz, attrs, origin=origin, dps=dps, gridRes=res)
        added = c.close_ball(16)
        m = c.info().numberOfVoxels
        bk.emit(base, op="close_ball16", added=added, voxels_closed=m)
        d2, near = mv.DeviceArray(max(n, m), np.uint64), mv.DeviceArray(max(n, m), np.uint32)
        r = {}
        measure("between_a_to_closed", lambda: r.update(a.nearest_between_device(c, capacity=n, dist2=d2, nearest=near)))
        bk.emit(base, op="between_a_to_closed_result", **r)
        measure("between_closed_to_a", lambda: r.update(c.nearest_between_device(a, capacity=m, dist2=d2, nearest=near)))
        bk.emit(base, op="between_closed_to_a_result", **r)
        cx, _ = bk.snapshot(mv, c)
        # (the ball closing already gives a new cell the bytes of its nearest voxel: with the closed set's own bytes the transfer would find nothing to change.
        # The clean geometry of the use case has no colours yet: a flat grey)
        grey = mv.DeviceArray.from_host(np.tile(np.array([128, 128, 128, 255, 0, 0, 0, 255], np.uint8), (m, 1)))
        reset = lambda: c.edit_voxels(cx, grey)
        out = []
        measure("transfer_closed_from_a", lambda: out.append(c.transfer_attributes(a)), before=reset)
        bk.emit(base, op="transfer_closed_from_a_result", changed=out[-1][0], beyond=out[-1][1])
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
            bk.emit(base, op="nearest_voxels_random_rate", queries_per_s=args.queries / (ms * 1e-3))
    elif op == "band":
        measure("yardstick_distance_cells_64_count", lambda: a.distance_cells_device(64), figures=False, radius2=64)
    elif op == "noseed":  # one call each: the figures are what is wanted
        a.nearest_between_device(a, (8, 0, 0))
        bk.emit(base, op="between_shift8_summary_figures", **query_figures(mv))
        q = random_queries()
        a.nearest_voxels_device(args.queries, q)
        bk.emit(base, op="nearest_voxels_random_figures", **query_figures(mv))


def line(r):
    what = "%9.2f ms" % r["ms"] if "ms" in r else r.get("refused") or r.get("skipped") or r.get("failed") or ""
    return "%-7s %5s %-36s seed %-5s %10s voxels  %s  %s" % (r.get("scene", r.get("step")), r.get("grid", ""), r.get("op", ""), r.get("seed", ""), r.get("voxels", ""), what,
                                                             "visits/query %.1f most %d" % (r["visits_per_query"], r["most_visits"]) if "visits_per_query" in r else "")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=bk.parse_scenes, default="dragon:2048,tunnel:4096")
    ap.add_argument("--ops", default="shift,closed,random,band,noseed")
    ap.add_argument("--queries", type=int, default=1 << 24)
    ap.add_argument("--variant", default=os.path.join(bk.ROOT, "build", "ab", "libmvrt_exp.so"))
    bk.add_step_args(ap, reps=5, warmup=1, step_timeout=420)
    args = ap.parse_args()
    if args.step:
        return step(args)
    steps = ["%s:%d:%s" % (name, res, op) for name, res in args.scenes for op in args.ops.split(",")]
    noseed = lambda s: s.endswith(":noseed")
    no_variant = "no experiment build at %s (tools/build_variant.sh exp)" % os.path.relpath(args.variant, bk.ROOT)
    rows, rc = bk.run_steps(__file__, steps, lambda s: bk.flags(args, "reps", "warmup", "queries"), args.step_timeout, args.out,
                            env_for=lambda s: dict(MVRT_LIB=args.variant, MVRT_NEAREST_QUERY_SEED="0") if noseed(s) else None,
                            skipped=lambda s: no_variant if noseed(s) and not os.path.exists(args.variant) else None)
    bk.print_table(rows, line)
    return rc


if __name__ == "__main__":
    sys.exit(main())
