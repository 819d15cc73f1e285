"""The host-callable arithmetic of the coarsening without a GPU: coarseHead on shifted codes and the per-cell finish (coarseKeep, coarseMean, coarseAttrib,
coarseMaxCount) of csrc/voxel_passes.h, which the kernels of csrc/kernels_coarsen.hip are built on, against brute force -- sums of 255 * (2^32 - 2), counts at
8^20, shifts of 3, 33 and 60 bits.  tests/hip/coarsen_host.hip is a program of its own that makes no HIP call; it is compiled for the host with hipcc and run
here."""
import os

import pytest

import common


@pytest.mark.skipif(not os.path.exists(common.HIPCC), reason="no hipcc")
def test_coarsen_helpers_against_brute_force(tmp_path):
    common.run_host_probe(tmp_path, "coarsen_host", "coarsen host checks ok", timeout=120)
