"""The shared pieces of the voxel-set passes without a GPU: the Morton codec, lowerBound and popcount8 of csrc/mvrt_common.h and findRun / nthSetBit of
csrc/voxel_passes.h, which the emit kernels of the surface, the fill and the walk are built on, against brute force.  tests/hip/voxel_passes_host.hip is a
program of its own that makes no HIP call; it is compiled for the host with hipcc and run here."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PROBE = os.path.join(ROOT, "tests", "hip", "voxel_passes_host.hip")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_host_callable_helpers_against_brute_force(tmp_path):
    exe = str(tmp_path / "voxel_passes_host")
    # (the program has no kernel: the host pass is all of it)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-O2", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-Wno-unused-result", PROBE, "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "voxel passes host checks ok" in r.stdout
