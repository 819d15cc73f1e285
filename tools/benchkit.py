"""What the tools/*_bench.py scripts share: the scenes, the timing loop, the JSON rows and the step driver.  Stated once, here.

A STEP is one child process of the tool's own script (`--step NAME`): it builds its octree for itself, prints one JSON row per measurement and exits.
run_steps() starts the steps one after the other, each under `timeout -k 10 --step-timeout` (TERM at the limit, KILL 10 s later), and keeps their rows.  The
first step that fails, is killed or runs out of time ENDS THE RUN: nothing more is started on the GPU behind it.  What was measured up to there is in --out,
which is rewritten after every step.

timed_each() is the one clock.  Two conventions, by flag, never mixed inside one tool:
  blocking calls         per call: before(), synchronize(), clock around fn(); the first `warmup` calls of the same loop are discarded
  asynchronous launches  warmup_first: `warmup` bare calls of fn, then per call: synchronize(), clock around fn() + synchronize() (sync_after)
This module imports nothing of the package until a function is handed `mv`, so that the driver can be tested without a GPU."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SCENE_GRID = {"dragon": 2048, "tunnel": 4096}


def parse_scenes(text, grids=SCENE_GRID):
    """"dragon,tunnel:4096,dragon:64" -> [("dragon", 2048), ("tunnel", 4096), ("dragon", 64)]; for argparse's type="""
    out = []
    for item in text.split(","):
        name, _, grid = item.partition(":")
        if name not in grids:
            raise argparse.ArgumentTypeError("unknown scene %r (one of %s)" % (name, ", ".join(grids)))
        if grid and not (grid.isdigit() and int(grid) > 0 and int(grid) & (int(grid) - 1) == 0):
            raise argparse.ArgumentTypeError("the grid of %r is not a power of two" % item)
        out.append((name, int(grid) if grid else grids[name]))
    return out


def built(mv, name, res):
    """-> (octree of the procedural scene at res^3, origin, dps)"""
    from massivevoxelraytracing_amd import scenes
    verts, cols, emis = scenes.SCENES[name](1.0)
    origin, dps = scenes.bounding_grid(verts, res)
    svo = mv.IntersectorOctreeGPU()
    svo.build(verts, cols, emis, None, origin, dps, res)
    return svo, origin, dps


def snapshot(mv, svo):
    """-> the octree's voxel list (xyz, attrs) in device arrays"""
    n = svo.info().numberOfVoxels
    xyz, attrs = mv.DeviceArray((n, 3), np.uint32), mv.DeviceArray((n, 8), np.uint8)
    mv._check(mv.lib().mvrt_svo_read_voxels(svo._h, xyz.ptr, attrs.ptr, None))
    return xyz, attrs


def peak_of(mv, fn):
    """the most bytes the library held during fn beyond what it held before"""
    held = mv.allocation_state()[1]
    mv.peak_bytes(reset=True)
    fn()
    return mv.peak_bytes() - held


def timed_each(mv, fns, reps, warmup, before=None, after=None, sync_after=False, warmup_first=False):
    """the calls of fns alternate (f0, f1, f0, f1, ...); -> per fn (median, all) in ms.  after(j, result) runs once the clock of a call of fns[j] has stopped"""
    ts = [[] for _ in fns]
    if warmup_first:
        for _ in range(warmup):
            for fn in fns:
                fn()
        warmup = 0
    for i in range(warmup + reps):
        for j, fn in enumerate(fns):
            if before:
                before()
            mv.synchronize()
            t0 = time.perf_counter()
            result = fn()
            if sync_after:
                mv.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            if i >= warmup:
                ts[j].append(ms)
            if after:
                after(j, result)
    return [(float(np.median(t)), t) for t in ts]


def timed(mv, fn, reps, warmup, **how):
    """one fn through timed_each -> (median, all) in ms"""
    return timed_each(mv, [fn], reps, warmup, **how)[0]


def timed_async(mv, fn, reps, warmup):
    """asynchronous launches of one fn: warm-ups first, the clock between device synchronisations -> (median, all) in ms"""
    return timed(mv, fn, reps, warmup, sync_after=True, warmup_first=True)


def emit(base, **kw):
    """one row: one JSON line on stdout, at once"""
    print(json.dumps(dict(base, **kw)), flush=True)


def timed_or_refused(mv, base, label, fn, reps, warmup, before=None, **kw):
    """blocking calls of fn as one row with the last call's result -> that result; a call the library refuses is one `refused` row with its message -> None"""
    last = []
    try:
        ms, ts = timed(mv, fn, reps, warmup, before=before, after=lambda j, result: last.append(result))
    except mv.MvrtError as err:
        emit(base, op=label, refused=str(err), **kw)
        return None
    emit(base, op=label, ms=ms, all_ms=ts, result=last[-1], **kw)
    return last[-1]


def brief(row):
    """a row as the driver echoes it where all_ms would drown the line"""
    return json.dumps({k: v for k, v in row.items() if k != "all_ms"})


def add_step_args(ap, reps, warmup, step_timeout, out=None):
    ap.add_argument("--reps", type=int, default=reps)
    ap.add_argument("--warmup", type=int, default=warmup)
    ap.add_argument("--step-timeout", type=int, default=step_timeout)
    ap.add_argument("--out", default=out)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)


def flags(args, *names):
    """("reps", "close_radius") -> ["--reps", "5", "--close-radius", "16"]: a tool's own settings on their way to its steps"""
    return [s for n in names for s in ("--" + n.replace("_", "-"), str(getattr(args, n)))]


def run_steps(script, steps, child_args, step_timeout, out=None, env_for=None, failed_fields=None, skipped=None, echo=None):
    """the driver (see the head of this file) -> (rows, 0 or 1).  env_for(step) -> variables on top of the environment; skipped(step) -> why no child is
    started for it (a row says so), or None; echo(row) -> the line printed for a row in place of the child's own"""
    rows, rc = [], 0

    def save():
        if out:
            with open(out, "w") as f:
                json.dump(rows, f, indent=1)

    for step in steps:
        why = skipped(step) if skipped else None
        if why:
            rows.append(dict(step=step, skipped=why))
            continue
        cmd = ["timeout", "-k", "10", str(step_timeout), sys.executable, os.path.abspath(script), "--step", step, *child_args(step)]
        print("step", step, flush=True)
        child = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True, env=dict(os.environ, **(env_for(step) or {})) if env_for else None)
        for line in child.stdout:
            if line.startswith("{"):
                rows.append(json.loads(line))
                print(echo(rows[-1]) if echo else line.rstrip("\n"), flush=True)
        status = child.wait()
        if status != 0:
            rows.append(dict(step=step, failed="no result within %d s" % step_timeout if status in (124, 137) else "exit status %d" % status,
                             **(failed_fields(step) if failed_fields else {})))
            rc = 1
            break  # nothing more is started on the GPU behind a step that failed
        save()
    save()
    return rows, rc


def print_table(rows, line):
    for r in rows:
        print(line(r), file=sys.stderr)
