"""Distance-limited rays and the occlusion bake, the parts that need no GPU: the direction table of mvrt_ao_directions against the oracle's sampleLambertian
on the Hammersley points, the refusals that happen on the host before any GPU call, and the three layers of the interface (header, binding, C++ mirror)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import common
import massivevoxelraytracing_amd as mv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# unit normals in the order of mvrt.h: 0 -Y, 1 +Y, 2 -Z, 3 +X, 4 +Z, 5 -X; the zeros are +0.0
NORMALS = np.array([(0, -1, 0), (0, 1, 0), (0, 0, -1), (1, 0, 0), (0, 0, 1), (-1, 0, 0)], np.float32)


def hammersley(K):
    k = np.arange(K)
    a = ((k.astype(np.float32) + np.float32(0.5)) / np.float32(K)).astype(np.float32)
    b = np.array([int(format(i, "032b")[::-1], 2) / 2.0 ** 32 for i in k], np.float32)  # base-2 radical inverse, exact for k < 2^24
    return a, b


def expected_directions(K):
    from oracle import oracle as O
    a, b = hammersley(K)
    return np.array([[O.sample_lambertian(float(a[k]), float(b[k]), NORMALS[d], math_mode=1) for k in range(K)] for d in range(6)], np.float32)


@pytest.mark.parametrize("K", [1, 2, 16, 64, 256])
def test_ao_directions_equal_the_oracle(K):
    got = mv.ao_directions(K)
    assert got.shape == (6, K, 3)
    assert np.array_equal(got.view(np.uint32), expected_directions(K).view(np.uint32))
    assert np.all((got * NORMALS[:, None, :]).sum(2) > 0)  # every direction leaves its face


def test_hammersley_points_are_exact():
    a, b = hammersley(256)
    assert np.array_equal(a.astype(np.float64), (np.arange(256) + 0.5) / 256) and b[1] == 0.5 and b[2] == 0.25 and b[255] == 255 / 256


def refused(rc, text):
    return rc != 0 and text in mv.lib().mvrt_last_error()


def test_refusals_need_no_gpu():
    """every rejected argument fails on the host before the handle is looked at: a null handle never gets a 'no octree' answer here"""
    lib = mv.lib()
    out = np.zeros(6 * 512 * 3, np.float32)
    for K in (0, 3, 512, -4):
        assert refused(lib.mvrt_ao_directions(K, out.ctypes.data), b"power of two")
        assert refused(lib.mvrt_svo_surface_ao(None, 1, out.ctypes.data, out.ctypes.data, K, 1.0, out.ctypes.data, None), b"power of two")
    assert refused(lib.mvrt_ao_directions(16, None), b"null output")
    for radius in (float("nan"), 0.0, -1.0, float("-inf")):
        assert refused(lib.mvrt_svo_surface_ao(None, 1, out.ctypes.data, out.ctypes.data, 16, radius, out.ctypes.data, None), b"radius")
    assert refused(lib.mvrt_svo_surface_ao(None, 1, out.ctypes.data, out.ctypes.data, 16, 1.0, None, None), b"null")
    assert refused(lib.mvrt_svo_surface_ao(None, 1, None, out.ctypes.data, 16, 1.0, out.ctypes.data, None), b"null")
    assert refused(lib.mvrt_svo_surface_ao(None, 1, out.ctypes.data, out.ctypes.data, 16, 1.0, out.ctypes.data, None), b"null handle")
    p = out.ctypes.data
    assert refused(lib.mvrt_trace_batch_range(None, 1, p, p, p, p, p, p, None, None, p, p, p, p, None), b"tMaxDev")
    assert refused(lib.mvrt_trace_batch_range(None, 1, p, p, p, p, p, p, None, p, None, p, p, p, None), b"t output")
    assert refused(lib.mvrt_trace_batch_range(None, 1, p, p, None, p, p, p, None, p, p, p, p, p, None), b"null ray array")
    assert refused(lib.mvrt_trace_batch_range(None, 1, p, p, p, p, p, p, None, p, p, p, p, p, None), b"no octree")
    with pytest.raises(mv.MvrtError, match="power of two"):
        mv.ao_directions(3)


def test_interface_is_declared_in_every_layer():
    header = open(os.path.join(ROOT, "include", "mvrt.h")).read()
    mirror = open(os.path.join(ROOT, "include", "mvrt", "IntersectorOctreeGPU.hpp")).read()
    device = open(os.path.join(ROOT, "include", "mvrt", "device.hpp")).read()
    for name in ("mvrt_trace_batch_range", "mvrt_ao_directions", "mvrt_svo_surface_ao"):
        assert name + "(" in header and name in mv.SIGNATURES and name + "(" in mirror
    for name in ("intersect_range", "intersect_range_device", "surface_ao", "surface_ao_device"):
        assert callable(getattr(mv.IntersectorOctreeGPU, name))
    assert callable(mv.ao_directions)
    for name in ("intersectRange(", "intersectRangeEx(", "occluded(", "template <bool RANGE>"):
        assert name in device
    assert "__FAST_MATH__" in device and "fp contract(off)" in device  # the refusal and the discipline are kept


def test_cpp_mirror_range_methods_compile_and_link(tmp_path):
    exe, libdir = common.compile_usage(tmp_path, "range_usage")
    out = subprocess.check_output([str(exe)], env=dict(os.environ, LD_LIBRARY_PATH=libdir + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", "")))
    assert b"usage" in out and b"directions 24" in out
    first = np.array(out.split(b"first ")[1].split(b")")[0].split(), np.float32)
    assert np.array_equal(first, mv.ao_directions(4)[0, 0])
