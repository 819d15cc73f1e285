"""The C calls behind the host-vector forms of the C++ mirror, pinned without a library: tests/cpp/mirror_calls.cpp includes include/mvrt/IntersectorOctreeGPU.hpp,
defines the mvrt_* entries itself as logging fakes and prints one line per call -- capacities, which pointers are null, which allocation each of the others is
and its size, the copies and the frees, in order.  tests/cpp/mirror_calls.txt is that text; a change of the header that moves, drops, adds or reorders a call
in any host-vector form shows as a difference."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_vector_forms_make_the_recorded_calls(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "mirror_calls"
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "mirror_calls.cpp"), "-o", str(exe)])
    got = subprocess.check_output([str(exe)])
    with open(os.path.join(ROOT, "tests", "cpp", "mirror_calls.txt"), "rb") as f:
        want = f.read()
    assert got == want
    assert got.count(b"\n") > 500 and b"?" not in got  # every pointer the fakes saw was null or one of the allocations
