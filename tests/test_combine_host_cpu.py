"""The host-callable helpers the two-set kernels are built on, without a GPU: the translation of a code by an integer offset (combineTranslate) against brute
force on grids of gridRes 2 and 4 for every offset in [-R, R]^3 and at the borders of the 2^21 grid, where nothing may be folded back, and the windowed partner
search (combineWindow / codeIndexInRange) against codeIndexIn on random sorted lists (csrc/voxel_passes.h).  tests/hip/combine_host.hip is a program of its own
that makes no HIP call; it is compiled for the host with hipcc and run here."""
import os

import pytest

import common


@pytest.mark.skipif(not os.path.exists(common.HIPCC), reason="no hipcc")
def test_combine_helpers_against_brute_force(tmp_path):
    common.run_host_probe(tmp_path, "combine_host", "combine host checks ok", timeout=120)
