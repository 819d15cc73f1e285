"""The cell-to-gap lookup of the exterior masks without a GPU: gapNodeOfCell and gapLength of csrc/voxel_passes.h, which the exterior-masks kernel asks once per
neighbour cell, against brute force -- by hand on every case of the rule (a cell before the first and behind the last voxel of the list, a voxel-free row, the
end runs, a true gap, adjacent voxels, a left neighbour in the previous row) and on every empty cell of random grids.  tests/hip/exterior_host.hip is a program
of its own that makes no HIP call; it is compiled for the host with hipcc and run here."""
import os

import pytest

import common


@pytest.mark.skipif(not os.path.exists(common.HIPCC), reason="no hipcc")
def test_cell_to_gap_against_brute_force(tmp_path):
    common.run_host_probe(tmp_path, "exterior_host", "exterior host checks ok", timeout=60)
