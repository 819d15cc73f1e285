"""The measurement tools on top of tools/benchkit.py, each through its real driver on a real scene at the smallest size: the dragon at 64^3 (6 levels), one
timed call, one step selected where the tool has a flag for it.  A tool must end with status 0, report no failed step, and every row that carries `ms` must
have exactly the keys of the rows with the same op in the committed profiles/<tool>.json (range_bench.py has no committed profile: its rows are written out
below from the script).  Rows that say `refused` or `skipped` are legitimate at this size (a 64^3 shell may enclose nothing): they carry the tool's base
fields.  What the figures measure is pinned by the call-order tests of tests/test_benchkit_cpu.py, not here."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_LIMIT = 60
SMALL = ["--reps", "1", "--warmup", "0"]
DRAGON = ["--scenes", "dragon:64"]

# tool -> (the fields every row of the tool carries, the arguments of each case)
TOOLS = {
    "ball": ("scene grid voxels", [DRAGON + ["--ops", "distance", "--radii", "1,9"], DRAGON + ["--ops", "close", "--close-radius", "9", "--cube-steps", "1"]]),
    "coarsen": ("scene grid voxels", [DRAGON]),
    "combine": ("scene grid voxels lib", [DRAGON + ["--ops", "listing"], DRAGON + ["--ops", "inplace", "--host-reps", "1"]]),
    "components": ("scene grid voxels", [DRAGON + ["--ops", "listings"], DRAGON + ["--ops", "keep", "--debris", "100"]]),
    "enclosed_nearest": ("scene grid voxels nCells nRegions", [DRAGON + ["--ops", op] for op in ("size", "list", "fill")]),
    "exterior": ("scene grid voxels nCells nRegions nFacesPlain lib round", [DRAGON + ["--no-fill-route"]]),
    "fill": ("scene grid voxels nCells nRegions", [DRAGON + ["--no-host-method"]]),
    "lod_cone": ("scene grid levels voxels size", [["--grids", "64", "--steps", s] for s in ("pyramid", "yardstick", "cone", "render")]),
    "morph": ("scene grid voxels element", [DRAGON + ["--elements", "faces", "--close-steps", "1", "--ops", op] for op in ("listings", "steps", "close")]),
    "nearest_query": ("scene grid voxels seed", [DRAGON + ["--queries", "4096", "--ops", op] for op in ("shift", "closed", "random", "band", "noseed")]),
    "range": ("scene grid", [["--grid", "64", "--steps", s] for s in ("unlimited", "limited", "ao")]),
    "resample": ("scene case src_grid grid voxels lib", [DRAGON + ["--cases", c] for c in ("identity", "turn90", "turn30", "magnify2")]),
    "surface": ("scene grid voxels nFaces nVertices", [DRAGON + ["--no-host-method"]]),
    "upload_walk": ("scene grid", [DRAGON + ["--no-pt"]]),
    "voxel_edit": ("scene grid", [DRAGON]),
}
STEP_TOOLS = set(TOOLS) - {"surface", "upload_walk", "voxel_edit"}
PROFILE = {"voxel_edit": "r05_voxel_edit_bench.json"}
RANGE_ROWS = {  # tools/range_bench.py, row by row
    "trace_batch": "op ms all_ms rays_per_s mean_descents hits scene grid rays n",
    "trace_batch_range": "op tMax ms all_ms rays_per_s mean_descents mean_descents_unlimited hits equal_to_filtered_trace_batch scene grid rays n",
    "surface_quads": "op ms all_ms scene grid voxels nFaces",
    "surface_ao": "op samples radius_voxels ms all_ms rays_per_s mean_open_fraction scene grid voxels nFaces",
}
CASES = [(tool, args) for tool, (_, cases) in TOOLS.items() for args in cases]


def expected_keys(tool):
    """op -> the key sets of the committed rows that carry `ms`"""
    if tool == "range":
        return {op: [set(keys.split())] for op, keys in RANGE_ROWS.items()}
    want = {}
    with open(os.path.join(ROOT, "profiles", PROFILE.get(tool, tool + "_bench.json"))) as f:
        for row in json.load(f):
            if "ms" in row and set(row) not in want.setdefault(row["op"], []):
                want[row["op"]].append(set(row))
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("tool,args", CASES, ids=["-".join([tool] + [a for a in args if not a.startswith("--") and a != "dragon:64"]) for tool, args in CASES])
def test_tool_at_the_smallest_size(tool, args, tmp_path):
    out = tmp_path / "rows.json"
    cmd = [sys.executable, os.path.join(ROOT, "tools", tool + "_bench.py"), *SMALL, *args, "--out", str(out)]
    if tool in STEP_TOOLS:
        cmd += ["--step-timeout", str(STEP_LIMIT)]
    done = subprocess.run(["timeout", "-k", "10", str(4 * STEP_LIMIT), *cmd], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
    rows = json.loads(out.read_text())
    assert rows and not [r for r in rows if "failed" in r], rows
    base, want = set(TOOLS[tool][0].split()), expected_keys(tool)
    for row in rows:
        if "step" in row:  # the driver's own row: a step for which no child was started
            assert set(row) == {"step", "skipped"}, row
            continue
        assert base <= set(row) and "op" in row, row  # (also all that is asked of a row that says `refused` or `skipped`, or that carries a ratio or a count)
        if "ms" in row:
            assert row["op"] in want, "%s: no committed row with op %s" % (tool, row["op"])
            assert set(row) in want[row["op"]], (row["op"], sorted(set(row) ^ want[row["op"]][0]))
            assert row["ms"] > 0 and len(row.get("all_ms", [0])) == 1
