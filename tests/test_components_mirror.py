"""The component interface without a GPU: the header, the Python table and the C++ mirror declare the two calls, and tests/cpp/components_usage.cpp, which pins
their C signatures, compiles and links against the library (it is run on a GPU by tests/test_gpu_components_app.py)."""
import os
import subprocess

import pytest

import common
import massivevoxelraytracing_amd as mv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("mvrt_svo_components", "mvrt_svo_keep_components")


def test_header_python_and_mirror_declare_the_interface():
    src = open(os.path.join(ROOT, "include", "mvrt.h")).read()
    for name in CALLS:
        assert name + "(" in src and name in mv.SIGNATURES
    assert len(mv.SIGNATURES["mvrt_svo_components"][1]) == 10 and len(mv.SIGNATURES["mvrt_svo_keep_components"][1]) == 7
    for name in ("components_device", "components", "keep_components"):
        assert callable(getattr(mv.IntersectorOctreeGPU, name))
    hpp = open(os.path.join(ROOT, "include", "mvrt", "IntersectorOctreeGPU.hpp")).read()
    for name in ("uint64_t components(", "void components(", "uint64_t keepComponents("):
        assert name in hpp


def test_refusals_that_need_no_gpu():
    """a null handle and an empty one are refused on the host, before any GPU work"""
    lib = mv.lib()
    assert lib.mvrt_svo_components(None, 0, None, 0, None, None, None, None, None, None) != 0 and b"null handle" in lib.mvrt_last_error()
    assert lib.mvrt_svo_keep_components(None, 0, 1, 0, None, None, None) != 0 and b"null handle" in lib.mvrt_last_error()
    svo = mv.IntersectorOctreeGPU()
    for call in (svo.components_device, svo.components, svo.keep_components):
        with pytest.raises(mv.MvrtError, match="no octree"):
            call()


def test_cpp_mirror_component_methods_compile_and_link(tmp_path):
    exe, libdir = common.compile_usage(tmp_path, "components_usage")
    out = subprocess.check_output([str(exe)], env=dict(os.environ, LD_LIBRARY_PATH=libdir + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", "")))
    assert b"usage" in out
