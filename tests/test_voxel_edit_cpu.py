"""Voxel-list input, edits and read-back (mvrt_svo_build_voxels / mvrt_svo_edit_voxels / mvrt_svo_read_voxels) without a GPU: the host-side argument
checks fail with the intended messages before any HIP call, and the C++ mirror's new methods compile and link."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import common
import massivevoxelraytracing_amd as mv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE_DEV = 0x1000  # never dereferenced: every case below fails before the first HIP call


@pytest.fixture()
def empty_handle():
    lib = mv.lib()
    h = C.c_void_p(0)
    assert lib.mvrt_svo_create(C.byref(h)) == 0  # host allocation only
    yield lib, h.value
    lib.mvrt_svo_destroy(h.value)


def _err(lib):
    return lib.mvrt_last_error().decode()


def test_build_voxels_rejects_bad_arguments_on_the_host(empty_handle):
    lib, h = empty_handle
    o = np.zeros(3, np.float32)
    op = o.ctypes.data_as(C.c_void_p)
    cases = [
        ((None, FAKE_DEV, None, 8, op, 0.1, 16, 0, None), "null handle"),
        ((h, None, None, 8, op, 0.1, 16, 0, None), "null coordinates"),
        ((h, FAKE_DEV, None, 0, op, 0.1, 16, 0, None), "voxel count 0 is not in [1, 2^32-2]"),
        ((h, FAKE_DEV, None, 2**32 - 1, op, 0.1, 16, 0, None), "is not in [1, 2^32-2]"),
        ((h, FAKE_DEV, None, 8, op, 0.1, 12, 0, None), "gridRes 12 is not a power of two in [2, 2^21]"),
        ((h, FAKE_DEV, None, 8, op, 0.1, 1, 0, None), "gridRes 1 is not a power of two"),
        ((h, FAKE_DEV, None, 8, op, 0.1, 1 << 22, 0, None), "gridRes 4194304 is not a power of two in [2, 2^21]"),
        ((h, FAKE_DEV, None, 8, op, 0.1, 16, 4, None), "unsupported flags 0x4"),
        ((h, FAKE_DEV, None, 8, op, 0.1, 16, 8, None), "unsupported flags 0x8"),
    ]
    for args, msg in cases:
        assert lib.mvrt_svo_build_voxels(*args) != 0
        assert "mvrt_svo_build_voxels" in _err(lib) and msg in _err(lib), (args, _err(lib))


def test_edit_and_read_need_a_built_octree(empty_handle):
    lib, h = empty_handle
    assert lib.mvrt_svo_edit_voxels(None, FAKE_DEV, None, None, 1, None) != 0
    assert "mvrt_svo_edit_voxels: null handle" in _err(lib)
    assert lib.mvrt_svo_edit_voxels(h, FAKE_DEV, None, None, 1, None) != 0
    assert "mvrt_svo_edit_voxels: no octree" in _err(lib)
    assert lib.mvrt_svo_read_voxels(None, FAKE_DEV, FAKE_DEV, None) != 0
    assert "mvrt_svo_read_voxels: null handle" in _err(lib)
    assert lib.mvrt_svo_read_voxels(h, FAKE_DEV, FAKE_DEV, None) != 0
    assert "mvrt_svo_read_voxels: no octree" in _err(lib)
    # the handle is still empty and usable
    i = mv.SvoInfo()
    assert lib.mvrt_svo_get_info(h, C.byref(i)) == 0
    assert (i.numberOfNodes, i.numberOfVoxels, i.totalDumpedVoxels) == (0, 0, 0)


def test_header_declares_the_voxel_list_interface():
    src = open(os.path.join(ROOT, "include", "mvrt.h")).read()
    for name in ("mvrt_svo_build_voxels", "mvrt_svo_edit_voxels", "mvrt_svo_read_voxels"):
        assert name + "(" in src and name in mv.SIGNATURES
    assert "#define MVRT_VOXEL_REMOVE 0" in src and "#define MVRT_VOXEL_SET 1" in src
    assert (mv.IntersectorOctreeGPU.VOXEL_REMOVE, mv.IntersectorOctreeGPU.VOXEL_SET) == (0, 1)


def test_cpp_mirror_voxel_methods_compile_and_link(tmp_path):
    exe, libdir = common.compile_usage(tmp_path, "voxel_edit_usage")
    out = subprocess.check_output([str(exe)], env=dict(os.environ, LD_LIBRARY_PATH=libdir + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", "")))
    assert b"usage" in out
