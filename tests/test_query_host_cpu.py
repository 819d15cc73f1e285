"""The nearest-voxel query without a GPU: tests/hip/query_host.hip runs nearestQueryWalk, the function every lane of csrc/kernels_query.hip runs
(csrc/voxel_passes.h), on the host against brute force in __int128 -- 160 random sets of 8^3 and 16^3 with queries inside the grid, on its border and up to 40
cells outside it, the single voxel, the two corners of the 2^21 grid queried from the far corner and from +-2^22 (d2 near 2^47), every maxDist2 in { 0, d2 - 1,
d2, d2 + 1 }, with and without the seed, and the strict-tie case, which a local copy with the pruning rule flipped to >= gets wrong.  The program is one of its
own that makes no HIP call; it is compiled for the host with hipcc, once plain and once with the address and undefined-behaviour sanitizers, and run here
directly."""
import os

import pytest

import common


@pytest.mark.skipif(not os.path.exists(common.HIPCC), reason="no hipcc")
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_query_walk_against_brute_force(tmp_path, sanitize):
    common.run_host_probe(tmp_path, "query_host", "query host checks ok", sanitize, timeout=300)
