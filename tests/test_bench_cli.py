"""bench.py's --dump-outputs and --full on CPU: the CPU-only mode (configs[0], --mode cpu-primary) writes the arrays of its last timed
frame, identical from run to run, within the 64 MB budget; a larger output is cut to one fixed, seeded sample of rows."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run_cpu_primary(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--mode", "cpu-primary", "--steps", "2", "--width", "64", "--height", "36",
           "--grid-res", "64", "--cpu-threads", "2", "--dump-outputs", str(out_dir)] + list(extra)
    line = json.loads(subprocess.check_output(cmd, timeout=300).decode().strip().split("\n")[-1])
    return line, {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


def test_dump_outputs_cpu_primary_repeatable(tmp_path):
    line, a = run_cpu_primary(tmp_path / "a")
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    _, b = run_cpu_primary(tmp_path / "b", "--full")
    assert sorted(a) == ["descents", "n_major", "rgba", "t", "v_index"]
    assert a["rgba"].shape == (64 * 36, 4) and a["t"].shape == (64 * 36,)
    for k in a:
        assert a[k].dtype in (np.float32, np.float64)
        assert np.array_equal(a[k], b[k])
    assert (a["rgba"][:, 3] == 255).all() and (a["t"] < 3e38).any()


def test_dump_outputs_budget_sample(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 200_000)
    n = 100_000
    t = np.arange(n, dtype=np.float32)
    idx = np.arange(n, dtype=np.uint32) * 3
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"t": t, "idx": idx})
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 200_000
    rows = np.load(tmp_path / "a" / "sample_rows.npy")
    assert rows.dtype == np.float64 and len(rows) > 0 and (np.diff(rows) > 0).all()
    assert np.array_equal(np.load(tmp_path / "a" / "t.npy"), rows.astype(np.float32))
    got_idx = np.load(tmp_path / "a" / "idx.npy")
    assert got_idx.dtype == np.float64 and np.array_equal(got_idx, rows * 3)
    for f in os.listdir(tmp_path / "a"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
