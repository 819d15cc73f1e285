"""The host-callable helpers the resampling kernels are built on, without a GPU: the point rule (resamplePoint) against 128-bit arithmetic at the limits of the
transform (|m| = 2^30, |t| = 2^52, c = 2^21 - 1, negative sums just below a multiple of 2^25), the box of a node (resampleBox) against brute force over all its
sample points for every node of 8^3 and 16^3 destination grids under random transforms, and the voxel test on that box, which never rejects a node that holds a
result cell (csrc/voxel_passes.h).  tests/hip/resample_host.hip is a program of its own that makes no HIP call; it is compiled for the host with hipcc, once plain and
once with the address and undefined-behaviour sanitizers -- the signed-overflow check is the point -- and run here directly."""
import os

import pytest

import common


@pytest.mark.skipif(not os.path.exists(common.HIPCC), reason="no hipcc")
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_resample_helpers_against_brute_force(tmp_path, sanitize):
    common.run_host_probe(tmp_path, "resample_host", "resample host checks ok", sanitize, timeout=300)
