"""The host-callable arithmetic of the round-offset passes without a GPU: the reach of a radius, the shift interval of an entry clipped to the grid up to gridRes
2^21, the shifted code and the packed key (ballReach, ballShiftRange, ballShifted, ballKey, ballShiftKey of csrc/voxel_passes.h), which the kernels of
csrc/kernels_ball.hip are built on, and the three passes run with them on the host, against brute force.  tests/hip/ball_host.hip is a program of its own that
makes no HIP call; it is compiled for the host with hipcc and run here."""
import os

import pytest

import common


@pytest.mark.skipif(not os.path.exists(common.HIPCC), reason="no hipcc")
def test_ball_helpers_against_brute_force(tmp_path):
    common.run_host_probe(tmp_path, "ball_host", "ball host checks ok", timeout=120)
