"""The host-callable helpers the component kernels are built on, without a GPU: the half of each structuring element (componentHalf), which must cover every
unordered adjacent pair exactly once, the index-returning search (codeIndexIn) against brute force on grids of gridRes 2 and 4, and the borders of the 2^21 grid,
where nothing may be folded back (csrc/voxel_passes.h).  tests/hip/components_host.hip is a program of its own that makes no HIP call; it is compiled for the host
with hipcc and run here."""
import os

import pytest

import common


@pytest.mark.skipif(not os.path.exists(common.HIPCC), reason="no hipcc")
def test_component_helpers_against_brute_force(tmp_path):
    common.run_host_probe(tmp_path, "components_host", "components host checks ok", timeout=120)
