"""The round-offset interface without a GPU: the header, the Python table and the C++ mirror declare the six calls, and tests/cpp/ball_usage.cpp compiles and
links against the library (it is run on a GPU by tests/test_gpu_ball_app.py)."""
import os
import subprocess

import pytest

import common
import massivevoxelraytracing_amd as mv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("mvrt_svo_distance_cells", "mvrt_svo_depth_voxels", "mvrt_svo_dilate_ball", "mvrt_svo_erode_ball", "mvrt_svo_close_ball", "mvrt_svo_open_ball")


def test_header_python_and_mirror_declare_the_interface():
    src = open(os.path.join(ROOT, "include", "mvrt.h")).read()
    for name in CALLS:
        assert name + "(" in src and name in mv.SIGNATURES
    for name in ("distance_cells_device", "distance_cells", "depth_voxels_device", "depth_voxels", "dilate_ball", "erode_ball", "close_ball", "open_ball"):
        assert callable(getattr(mv.IntersectorOctreeGPU, name))
    hpp = open(os.path.join(ROOT, "include", "mvrt", "IntersectorOctreeGPU.hpp")).read()
    for name in ("distanceCells(", "depthVoxels(", "dilateBall(", "erodeBall(", "closeBall(", "openBall("):
        assert name in hpp


def test_refusals_that_need_no_gpu():
    """a null handle and an empty one are refused on the host, before any GPU work"""
    lib = mv.lib()
    assert lib.mvrt_svo_dilate_ball(None, 1, None, None) != 0 and b"null handle" in lib.mvrt_last_error()
    assert lib.mvrt_svo_depth_voxels(None, 1, 0, None, None, None, None) != 0 and b"null handle" in lib.mvrt_last_error()
    svo = mv.IntersectorOctreeGPU()
    for call in (svo.distance_cells_device, svo.depth_voxels_device, svo.dilate_ball, svo.erode_ball, svo.close_ball, svo.open_ball):
        with pytest.raises(mv.MvrtError, match="no octree"):
            call()


def test_cpp_mirror_ball_methods_compile_and_link(tmp_path):
    exe, libdir = common.compile_usage(tmp_path, "ball_usage")
    out = subprocess.check_output([str(exe)], env=dict(os.environ, LD_LIBRARY_PATH=libdir + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", "")))
    assert b"usage" in out
