"""The host-callable arithmetic of the morphology passes without a GPU: the neighbour tables, the in-grid test up to gridRes 2^21 and the empty-neighbour masks
(morphOffset, morphNeighbour, codePresentIn, morphEmptyMask of csrc/voxel_passes.h), which the kernels of csrc/kernels_morph.hip are built on, against brute
force.  tests/hip/morph_host.hip is a program of its own that makes no HIP call; it is compiled for the host with hipcc and run here."""
import os

import pytest

import common


@pytest.mark.skipif(not os.path.exists(common.HIPCC), reason="no hipcc")
def test_morph_helpers_against_brute_force(tmp_path):
    common.run_host_probe(tmp_path, "morph_host", "morph host checks ok", timeout=120)
