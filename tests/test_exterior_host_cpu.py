"""The cell-to-gap lookup of the exterior masks without a GPU: gapNodeOfCell and gapLength of csrc/voxel_passes.h, which the exterior-masks kernel asks once per
neighbour cell, against brute force -- by hand on every case of the rule (a cell before the first and behind the last voxel of the list, a voxel-free row, the
end runs, a true gap, adjacent voxels, a left neighbour in the previous row) and on every empty cell of random grids.  tests/hip/exterior_host.hip is a program
of its own that makes no HIP call; it is compiled for the host with hipcc and run here."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PROBE = os.path.join(ROOT, "tests", "hip", "exterior_host.hip")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_cell_to_gap_against_brute_force(tmp_path):
    exe = str(tmp_path / "exterior_host")
    # (the program has no kernel: the host pass is all of it)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-O2", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-Wno-unused-result", PROBE, "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "exterior host checks ok" in r.stdout
