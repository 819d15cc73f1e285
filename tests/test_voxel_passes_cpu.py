"""The shared pieces of the voxel-set passes without a GPU: the Morton codec, lowerBound and popcount8 of csrc/mvrt_common.h and findRun / nthSetBit of
csrc/voxel_passes.h, which the emit kernels of the surface, the fill and the walk are built on, against brute force.  tests/hip/voxel_passes_host.hip is a
program of its own that makes no HIP call; it is compiled for the host with hipcc and run here."""
import os

import pytest

import common


@pytest.mark.skipif(not os.path.exists(common.HIPCC), reason="no hipcc")
def test_host_callable_helpers_against_brute_force(tmp_path):
    common.run_host_probe(tmp_path, "voxel_passes_host", "voxel passes host checks ok", timeout=60)
