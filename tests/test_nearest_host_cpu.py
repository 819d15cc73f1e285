"""The three passes over the gaps that give every enclosed cell its nearest voxel, without a GPU: tests/hip/nearest_host.hip runs them on the
host with the very functions the lanes of csrc/kernels_nearest.hip run (csrc/voxel_passes.h) and compares with brute force over all voxels on random shells of
8^3 to 16^3 with debris in their cavities (more than 20 000 enclosed cells), the cage and a shell at the far corner of the 2^21 grid; then the stop rule at its
boundary: a candidate at s^2 == d2 with a lower index wins, one at s^2 == d2 + 1 is not read (those cells are poisoned in the sanitizer build).  The program is
one of its own that makes no HIP call; it is compiled for the host with hipcc, once plain and once with the address and undefined-behaviour sanitizers, and run
here directly."""
import os

import pytest

import common


@pytest.mark.skipif(not os.path.exists(common.HIPCC), reason="no hipcc")
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_nearest_passes_against_brute_force(tmp_path, sanitize):
    common.run_host_probe(tmp_path, "nearest_host", "nearest host checks ok", sanitize, timeout=300)
