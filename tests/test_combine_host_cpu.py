"""The host-callable helpers the two-set kernels are built on, without a GPU: the translation of a code by an integer offset (combineTranslate) against brute
force on grids of gridRes 2 and 4 for every offset in [-R, R]^3 and at the borders of the 2^21 grid, where nothing may be folded back, and the windowed partner
search (combineWindow / codeIndexInRange) against codeIndexIn on random sorted lists (csrc/voxel_passes.h).  tests/hip/combine_host.hip is a program of its own
that makes no HIP call; it is compiled for the host with hipcc and run here."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PROBE = os.path.join(ROOT, "tests", "hip", "combine_host.hip")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_combine_helpers_against_brute_force(tmp_path):
    exe = str(tmp_path / "combine_host")
    # (the program has no kernel: the host pass is all of it)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-O2", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-Wno-unused-result", PROBE, "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "combine host checks ok" in r.stdout
