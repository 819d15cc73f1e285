"""The host-callable arithmetic of the round-offset passes without a GPU: the reach of a radius, the shift interval of an entry clipped to the grid up to gridRes
2^21, the shifted code and the packed key (ballReach, ballShiftRange, ballShifted, ballKey, ballShiftKey of csrc/voxel_passes.h), which the kernels of
csrc/kernels_ball.hip are built on, and the three passes run with them on the host, against brute force.  tests/hip/ball_host.hip is a program of its own that
makes no HIP call; it is compiled for the host with hipcc and run here."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PROBE = os.path.join(ROOT, "tests", "hip", "ball_host.hip")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_ball_helpers_against_brute_force(tmp_path):
    exe = str(tmp_path / "ball_host")
    # (the program has no kernel: the host pass is all of it)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-O2", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-Wno-unused-result", PROBE, "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ball host checks ok" in r.stdout
