"""The host-callable helpers the resampling kernels are built on, without a GPU: the point rule (resamplePoint) against 128-bit arithmetic at the limits of the
transform (|m| = 2^30, |t| = 2^52, c = 2^21 - 1, negative sums just below a multiple of 2^25), the box of a node (resampleBox) against brute force over all its
sample points for every node of 8^3 and 16^3 destination grids under random transforms, and the voxel test on that box, which never rejects a node that holds a
result cell (csrc/voxel_passes.h).  tests/hip/resample_host.hip is a program of its own that makes no HIP call; it is compiled for the host with hipcc, once plain and
once with the address and undefined-behaviour sanitizers -- the signed-overflow check is the point -- and run here directly."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PROBE = os.path.join(ROOT, "tests", "hip", "resample_host.hip")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_resample_helpers_against_brute_force(tmp_path, sanitize):
    exe = str(tmp_path / "resample_host")
    extra = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-Xarch_host", "-fno-omit-frame-pointer"] if sanitize else []
    # (the program has no kernel: the host pass is all of it)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-O1" if sanitize else "-O2", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function",
                        "-Wno-unused-result"] + extra + [PROBE, "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "resample host checks ok" in r.stdout and "runtime error" not in r.stderr
