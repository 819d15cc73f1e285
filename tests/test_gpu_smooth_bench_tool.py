"""tools/smooth_bench.py through its real driver at the smallest size, under the contract tests/test_gpu_bench_tools.py states for the other tools on top of
tools/benchkit.py: the dragon at 64^3, one timed call; status 0, no failed step, and every row that carries `ms` has exactly the keys of the rows with the same
op in the committed profiles/smooth_bench.json.  The row `iteration` carries a difference of two rows and no clock of its own: the tool's base fields."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_LIMIT = 60
BASE = set("scene grid voxels nFaces nVertices".split())


def expected_keys():
    want = {}
    with open(os.path.join(ROOT, "profiles", "smooth_bench.json")) as f:
        for row in json.load(f):
            if "ms" in row and set(row) not in want.setdefault(row["op"], []):
                want[row["op"]].append(set(row))
    return want


@pytest.mark.gpu
def test_tool_at_the_smallest_size(tmp_path):
    out = tmp_path / "rows.json"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "smooth_bench.py"), "--reps", "1", "--warmup", "0", "--scenes", "dragon:64", "--out", str(out), "--step-timeout", str(STEP_LIMIT)]
    done = subprocess.run(["timeout", "-k", "10", str(4 * STEP_LIMIT), *cmd], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
    rows = json.loads(out.read_text())
    assert rows and not [r for r in rows if "failed" in r], rows
    want = expected_keys()
    assert {"mesh", "smooth0", "smooth4", "smooth16", "host_route"} <= set(want)
    for row in rows:
        assert BASE <= set(row) and "op" in row, row
        if "ms" in row:
            assert row["op"] in want, "no committed row with op %s" % row["op"]
            assert set(row) in want[row["op"]], (row["op"], sorted(set(row) ^ want[row["op"]][0]))
            assert row["ms"] > 0 and len(row["all_ms"]) == 1
    ops = [r["op"] for r in rows]
    assert ops == ["mesh", "smooth0", "smooth4", "smooth16", "iteration", "host_route"]
    assert rows[-1]["equal_to_gpu"] is True and rows[2]["clamped"] == rows[4]["clamped"] and rows[4]["peak_bytes"] > 0
