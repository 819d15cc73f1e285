"""The smoothing interface without a GPU: the header, the Python table and the C++ mirror declare the two calls; null and empty handles, parameters outside
their ranges and non-zero reserved words are refused on the host with the field named; and tests/cpp/smooth_usage.cpp, which pins the C signatures, compiles
and links against the library (it is run on a GPU by tests/test_gpu_smooth_app.py)."""
import ctypes as C
import os
import subprocess

import pytest

import common
import massivevoxelraytracing_amd as mv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_python_and_mirror_declare_the_interface():
    src = open(os.path.join(ROOT, "include", "mvrt.h")).read()
    for name in ("mvrt_smooth_default_params", "mvrt_svo_surface_smooth"):
        assert name + "(" in src and name in mv.SIGNATURES
    assert "#define MVRT_SMOOTH_STEPS_PER_CELL 256" in src and "typedef struct mvrt_smooth_params" in src
    assert len(mv.SIGNATURES["mvrt_smooth_default_params"][1]) == 1 and len(mv.SIGNATURES["mvrt_svo_surface_smooth"][1]) == 15
    for name in ("surface_smooth_device", "surface_smooth"):
        assert callable(getattr(mv.IntersectorOctreeGPU, name))
    assert C.sizeof(mv.SmoothParams) == 32
    hpp = open(os.path.join(ROOT, "include", "mvrt", "IntersectorOctreeGPU.hpp")).read()
    for name in ("void surfaceSmooth(", "uint64_t surfaceSmooth(", "mvrt_smooth_params smoothDefaultParams("):
        assert name in hpp


def defaults():
    p = mv.SmoothParams()
    assert mv.lib().mvrt_smooth_default_params(C.byref(p)) == 0
    return p


def test_default_params():
    p = defaults()
    assert (p.iterations, p.weightEven, p.weightOdd, p.limit, list(p.reserved)) == (4, 256, 256, 127, [0, 0, 0, 0])
    assert mv.lib().mvrt_smooth_default_params(None) != 0 and b"null argument" in mv.lib().mvrt_last_error()


def test_refusals_that_need_no_gpu():
    lib = mv.lib()
    assert lib.mvrt_svo_surface_smooth(None, None, None, 0, 0, None, None, None, None, None, None, None, None, None, None) != 0 and b"null handle" in lib.mvrt_last_error()
    svo = mv.IntersectorOctreeGPU()
    for call in (svo.surface_smooth_device, svo.surface_smooth):
        with pytest.raises(mv.MvrtError, match="no octree"):
            call()
    with pytest.raises(mv.MvrtError, match="no octree"):
        svo.surface_smooth_device(defaults())  # parameters within their ranges pass, the limits included
    for field, values in (("iterations", (-1, 257)), ("weightEven", (-257, 257)), ("weightOdd", (-257, 257)), ("limit", (-1, 129))):
        for v in values:
            p = defaults()
            setattr(p, field, v)
            with pytest.raises(mv.MvrtError, match=r"%s %d outside" % (field, v)):
                svo.surface_smooth_device(p)
        for v in {"iterations": (0, 256), "weightEven": (-256, 256), "weightOdd": (-256, 256), "limit": (0, 128)}[field]:
            p = defaults()
            setattr(p, field, v)
            with pytest.raises(mv.MvrtError, match="no octree"):
                svo.surface_smooth_device(p)
    for k in range(4):
        p = defaults()
        p.reserved[k] = 1 << k
        with pytest.raises(mv.MvrtError, match=r"reserved\[%d\]" % k):
            svo.surface_smooth_device(p)


def test_cpp_mirror_smooth_methods_compile_and_link(tmp_path):
    exe, libdir = common.compile_usage(tmp_path, "smooth_usage")
    out = subprocess.check_output([str(exe)], env=dict(os.environ, LD_LIBRARY_PATH=libdir + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", "")))
    assert b"usage" in out
