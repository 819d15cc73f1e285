"""tools/benchkit.py without a GPU: the step driver on stub step scripts (order, the first-failure rule, the time limit, --out, skipping, per-step extras), the
timing loop on a fake device (the call order of each form), parse_scenes, and that no tool keeps a copy of what benchkit states."""
import argparse
import glob
import json
import os
import sys
import time
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import benchkit as bk  # noqa: E402

STUB = """import json, os, sys, time
step = sys.argv[sys.argv.index("--step") + 1]
here = os.path.dirname(os.path.abspath(__file__))
def row(**kw):
    print(json.dumps(dict(kw, step_of=step)), flush=True)
if step in ("a", "b"):
    row(n=1)
    print("not a row")
    row(n=2)
elif step == "c":
    row(n=1)
    sys.exit(3)
elif step == "sleep":
    time.sleep(30)
elif step == "env":
    row(var=os.environ.get("BENCHKIT_STUB"), args=sys.argv[3:])
else:
    open(os.path.join(here, "started_" + step), "w").close()
    row(n=1)
"""


@pytest.fixture
def stub(tmp_path):
    path = tmp_path / "stub_bench.py"
    path.write_text(STUB)
    return str(path)


def test_steps_in_order_and_nothing_behind_the_first_failure(stub, tmp_path, capfd):
    out = tmp_path / "rows.json"
    rows, rc = bk.run_steps(stub, ["a", "b", "c", "d"], lambda s: [], 60, out=str(out))
    want = [dict(n=1, step_of="a"), dict(n=2, step_of="a"), dict(n=1, step_of="b"), dict(n=2, step_of="b"), dict(n=1, step_of="c"), dict(step="c", failed="exit status 3")]
    assert rows == want and rc == 1
    assert not (tmp_path / "started_d").exists()
    assert json.loads(out.read_text()) == want
    echoed = [json.loads(line) for line in capfd.readouterr().out.splitlines() if line.startswith("{")]
    assert echoed == want[:5]  # every row is printed again, the non-JSON line is not a row


def test_all_steps_pass(stub, tmp_path):
    out = tmp_path / "rows.json"
    rows, rc = bk.run_steps(stub, ["a", "d"], lambda s: [], 60, out=str(out))
    assert rc == 0 and [r["step_of"] for r in rows] == ["a", "a", "d"] and (tmp_path / "started_d").exists()
    assert json.loads(out.read_text()) == rows


def test_out_is_written_after_every_step(stub, tmp_path):
    """a run that is cut off leaves what it measured: when the second step starts, the first step's rows are in the file already"""
    out = tmp_path / "rows.json"
    seen = []

    def child_args(step):
        seen.append(json.loads(out.read_text()) if out.exists() else None)
        return []

    bk.run_steps(stub, ["a", "b"], child_args, 60, out=str(out))
    assert seen == [None, [dict(n=1, step_of="a"), dict(n=2, step_of="a")]]


def test_time_limit_ends_the_step_and_the_run(stub, tmp_path):
    t0 = time.perf_counter()
    rows, rc = bk.run_steps(stub, ["a", "sleep", "d"], lambda s: [], 1)
    assert time.perf_counter() - t0 < 15  # ended by the limit (TERM after 1 s), not waited for: the stub would sleep 30 s
    assert rows[-1] == dict(step="sleep", failed="no result within 1 s") and rc == 1 and len(rows) == 3
    assert not (tmp_path / "started_d").exists()


def test_skipping_and_per_step_extras(stub, tmp_path):
    rows, rc = bk.run_steps(stub, ["env", "d", "c", "a"], lambda s: ["--reps", "2"] if s == "env" else [], 60,
                            env_for=lambda s: dict(BENCHKIT_STUB="for " + s) if s == "env" else None, failed_fields=lambda s: dict(lib="of " + s),
                            skipped=lambda s: "no such build" if s == "d" else None)
    assert rows == [dict(var="for env", args=["--reps", "2"], step_of="env"), dict(step="d", skipped="no such build"), dict(n=1, step_of="c"),
                    dict(step="c", failed="exit status 3", lib="of c")]
    assert rc == 1 and not (tmp_path / "started_d").exists()


def test_echo_replaces_the_printed_line(stub, capfd):
    bk.run_steps(stub, ["a"], lambda s: [], 60, echo=lambda row: "ROW %d" % row["n"])
    assert [line for line in capfd.readouterr().out.splitlines() if line.startswith("ROW")] == ["ROW 1", "ROW 2"]
    assert json.loads(bk.brief(dict(op="x", ms=1.0, all_ms=[1.0, 2.0]))) == dict(op="x", ms=1.0)


class FakeDevice:
    class MvrtError(RuntimeError):
        pass

    def __init__(self):
        self.log = []

    def synchronize(self):
        self.log.append("sync")

    def call(self, name, result=None, takes=None):
        def fn():
            self.log.append(name)
            if takes:
                takes[0][0] += takes.pop(1)
            return result
        return fn


@pytest.fixture
def ticking(monkeypatch):
    """benchkit's clock under the test's hand: each call of a fn made with takes=ticking(seconds, ...) advances it by the next of them"""
    now = [0.0]
    monkeypatch.setattr(bk, "time", types.SimpleNamespace(perf_counter=lambda: now[0]))
    return lambda *seconds: [now] + list(seconds)


def test_blocking_form(ticking):
    mv = FakeDevice()
    clock = ticking(1.0, 2.0, 0.003, 0.001, 0.002)
    ms, ts = bk.timed(mv, mv.call("fn", takes=clock), 3, 2, before=mv.call("before"))
    assert mv.log == ["before", "sync", "fn"] * 5
    assert ts == pytest.approx([3.0, 1.0, 2.0]) and ms == pytest.approx(2.0)  # the first two calls are discarded, the median of the rest
    mv.log.clear()
    bk.timed(mv, mv.call("fn"), 1, 1)
    assert mv.log == ["sync", "fn"] * 2


def test_asynchronous_form(ticking):
    mv = FakeDevice()
    clock = ticking(5.0, 5.0, 0.004, 0.002)
    ms, ts = bk.timed_async(mv, mv.call("fn", takes=clock), 2, 2)
    assert mv.log == ["fn", "fn"] + ["sync", "fn", "sync"] * 2
    assert ts == pytest.approx([4.0, 2.0]) and ms == pytest.approx(3.0)
    mv.log.clear()
    bk.timed(mv, mv.call("fn"), 2, 1, warmup_first=True)  # blocking calls, warm-ups first (surface_bench)
    assert mv.log == ["fn"] + ["sync", "fn"] * 2


def test_alternating_form(ticking):
    mv = FakeDevice()
    clock = ticking(9.0, 9.0, 0.001, 0.010, 0.003, 0.030)
    seen = []
    (ms0, ts0), (ms1, ts1) = bk.timed_each(mv, [mv.call("f0", "r0", clock), mv.call("f1", "r1", clock)], 2, 1, before=mv.call("before"),
                                           after=lambda j, result: seen.append((j, result, len(mv.log))))
    assert mv.log == ["before", "sync", "f0", "before", "sync", "f1"] * 3
    assert ts0 == pytest.approx([1.0, 3.0]) and ts1 == pytest.approx([10.0, 30.0]) and (ms0, ms1) == pytest.approx((2.0, 20.0))
    assert seen == [(j, "r%d" % j, 3 * k) for k, j in zip(range(1, 7), [0, 1] * 3)]  # after every call, before the next one's `before`


def test_refusal_wrapper(capfd):
    mv = FakeDevice()
    base = dict(scene="s")
    assert bk.timed_or_refused(mv, base, "count", mv.call("fn", 7), 2, 1, before=mv.call("before"), element="cube") == 7
    assert mv.log == ["before", "sync", "fn"] * 3
    row, = [json.loads(line) for line in capfd.readouterr().out.splitlines()]
    assert set(row) == {"scene", "op", "ms", "all_ms", "result", "element"} and row["result"] == 7 and row["op"] == "count" and len(row["all_ms"]) == 2

    def refuses():
        raise mv.MvrtError("too many cells")

    assert bk.timed_or_refused(mv, base, "list", refuses, 2, 1, element="cube") is None
    row, = [json.loads(line) for line in capfd.readouterr().out.splitlines()]
    assert row == dict(scene="s", op="list", refused="too many cells", element="cube")


def test_emit_is_one_json_line(capfd):
    bk.emit(dict(scene="dragon", grid=64), op="x", ms=1.5)
    assert capfd.readouterr().out == json.dumps(dict(scene="dragon", grid=64, op="x", ms=1.5)) + "\n"


def test_parse_scenes():
    assert bk.parse_scenes("dragon") == [("dragon", 2048)]
    assert bk.parse_scenes("tunnel:64") == [("tunnel", 64)]
    assert bk.parse_scenes("dragon,tunnel:4096,dragon:64") == [("dragon", 2048), ("tunnel", 4096), ("dragon", 64)]
    assert bk.parse_scenes("rtcamp,dragon:128", dict(dragon=2048, rtcamp=4096)) == [("rtcamp", 4096), ("dragon", 128)]
    for bad in ("bunny", "dragon,bunny:64", "dragon:100", "dragon:0", "dragon:-64", "dragon:x", ""):
        with pytest.raises(argparse.ArgumentTypeError):
            bk.parse_scenes(bad)
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=bk.parse_scenes, default="dragon,tunnel")
    bk.add_step_args(ap, reps=3, warmup=1, step_timeout=420)
    args = ap.parse_args([])
    assert args.scenes == [("dragon", 2048), ("tunnel", 4096)] and (args.reps, args.warmup, args.step_timeout, args.out, args.step) == (3, 1, 420, None, None)
    assert bk.flags(ap.parse_args(["--reps", "7"]), "reps", "step_timeout") == ["--reps", "7", "--step-timeout", "420"]
    with pytest.raises(SystemExit):
        ap.parse_args(["--scenes", "dragon:48"])


def test_no_copy_left_behind():
    """the point of benchkit: these exist once"""
    texts = {os.path.basename(p): open(p).read() for p in glob.glob(os.path.join(ROOT, "tools", "*.py"))}
    assert len(texts) > 16
    for needle in ("def timed", "def built", "def snapshot", "def peak_of", "GRID = {"):
        assert [name for name, text in sorted(texts.items()) if needle in text] == ["benchkit.py"], needle
    assert not [name for name, text in texts.items() if "TimeoutExpired" in text]  # the limit is `timeout -k 10` everywhere: TERM, then KILL
