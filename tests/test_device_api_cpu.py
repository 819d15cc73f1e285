"""The public device API (include/mvrt/device.hpp + mvrt_svo_device_view) without a GPU: the header compiles for gfx950 under a
user's flags and refuses -ffast-math, its code does not depend on the contraction flag, mvrt.h stays plain C/C++, and the view
entry point validates its arguments before touching the GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import massivevoxelraytracing_amd as mv
import reference_pins as R
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PROBE = os.path.join(ROOT, "tests", "hip", "device_api_probe.hip")
INC = os.path.join(ROOT, "include")

needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")


def hipcc(args):
    return subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", INC] + args, capture_output=True, text=True)


@needs_hipcc
@pytest.mark.parametrize("flags", [[], ["-ffp-contract=on"]])
def test_probe_compiles_warning_free_in_both_passes(tmp_path, flags):
    r = hipcc(["-c", "-Wall", "-Werror"] + flags + [PROBE, "-o", str(tmp_path / "probe.o")])
    assert r.returncode == 0, r.stderr


@needs_hipcc
def test_fast_math_is_refused_with_the_headers_message(tmp_path):
    r = hipcc(["-c", "-ffast-math", PROBE, "-o", str(tmp_path / "probe.o")])
    assert r.returncode != 0
    assert "mvrt/device.hpp: -ffast-math is not supported" in r.stderr


def device_isa(tmp_path, flags):
    out = tmp_path / ("probe%s.s" % "".join(flags).replace("=", "_"))
    r = hipcc(["--cuda-device-only", "-S"] + flags + [PROBE, "-o", str(out)])
    assert r.returncode == 0, r.stderr
    text = out.read_text()
    return re.sub(r"__hip_cuid_[0-9a-f]+", "CUID", text)  # (a per-compilation id)


@needs_hipcc
def test_device_code_is_the_uncontracted_code_under_the_default_flags_and_contract_on(tmp_path):
    """the library is built with -ffp-contract=off; the header's pragmas give the SAME gfx950 code under hipcc's default and -ffp-contract=on"""
    off = device_isa(tmp_path, ["-ffp-contract=off"])
    assert "kProbeTrace" in off
    assert device_isa(tmp_path, []) == off
    assert device_isa(tmp_path, ["-ffp-contract=on"]) == off


@needs_hipcc
@pytest.mark.parametrize("flags", [[], ["-ffp-contract=on"]], ids=["default", "contract_on"])
def test_host_side_camera_equals_the_compiled_reference(tmp_path, flags):
    """mvrt::CameraPinhole::shoot / shootThinLens are __host__ __device__: their host side, built under a user's flags, gives the compiled reference's rays
    bit for bit (or its stored digests) on the camera inputs of tests/test_reference_pins_cpu.py.  probe_camera_host makes no HIP call."""
    so = tmp_path / "probe_host.so"
    r = hipcc(["-fPIC", "-shared"] + flags + [PROBE, "-o", str(so)])
    assert r.returncode == 0, r.stderr
    lib = ctypes.CDLL(str(so))
    lib.probe_camera_host.restype = None
    lib.probe_camera_host.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    render = R.load_render(O, tree_decides=True)
    px, fl = R.camera_rays()
    for name, cam in R.cameras().items():
        for thin in (0, 1):
            ro, rd = np.zeros((len(px), 3), np.float32), np.zeros((len(px), 3), np.float32)
            lib.probe_camera_host(cam.ctypes.data, len(px), px.ctypes.data, fl.ctypes.data, thin, ro.ctypes.data, rd.ctypes.data)
            R.check("render/camera/%s/%d" % (name, thin), [ro, rd], render, lambda r: list(r.camera_shoot(cam, px, fl, bool(thin))))


def test_mvrt_h_compiles_as_plain_c_and_cpp(tmp_path):
    for cc, ext, std in (("gcc", "c", "-std=c11"), ("g++", "cpp", "-std=c++17")):
        exe = shutil.which(cc)
        if exe is None:
            pytest.skip("no " + cc)
        src = tmp_path / ("view." + ext)
        src.write_text('#include "mvrt.h"\nint f( const mvrt_svo* s ) { mvrt_device_octree v; return mvrt_svo_device_view( s, &v ) + (int)sizeof( v ); }\n')
        r = subprocess.run([exe, std, "-Wall", "-Werror", "-I", INC, "-c", str(src), "-o", str(tmp_path / ("view_%s.o" % ext))], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_device_view_of_an_empty_handle_fails_with_text():
    lib = mv.lib()
    svo = mv.IntersectorOctreeGPU()  # mvrt_svo_create allocates no device memory
    v = mv.DeviceOctree()
    assert lib.mvrt_svo_device_view(svo._h, ctypes.byref(v)) != 0
    assert b"no octree" in lib.mvrt_last_error()
    assert lib.mvrt_svo_device_view(None, ctypes.byref(v)) != 0
    assert b"null argument" in lib.mvrt_last_error()
    with pytest.raises(mv.MvrtError, match="no octree"):
        svo.device_view()


def test_ctypes_struct_matches_the_header():
    assert ctypes.sizeof(mv.DeviceOctree) == 128
    header = open(os.path.join(INC, "mvrt.h")).read()
    assert "sizeof( mvrt_device_octree ) == 128" in header
    for name, off in (("nodes", 8), ("cellEntries", 56), ("lower", 64), ("emissionScale", 92), ("levels", 100), ("cellBits", 124)):
        assert getattr(mv.DeviceOctree, name).offset == off, name
        assert "__builtin_offsetof( mvrt_device_octree, %s ) == %d" % (name, off) in header
