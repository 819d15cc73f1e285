"""The two-set interface: the header, the Python table and the C++ mirror declare the two calls, and tests/cpp/combine_usage.cpp, which pins their C
signatures, compiles and links against the library -- without a GPU.  On a GPU the program is run, and every line it prints is compared with what the Python
wrapper and the model of tests/combine_expected.py give for the same two sets."""
import os
import subprocess

import numpy as np
import pytest

import common
import combine_expected as E
import massivevoxelraytracing_amd as mv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("mvrt_svo_combine_voxels", "mvrt_svo_combine")


def test_header_python_and_mirror_declare_the_interface():
    src = open(os.path.join(ROOT, "include", "mvrt.h")).read()
    for name in CALLS:
        assert name + "(" in src and name in mv.SIGNATURES
    assert len(mv.SIGNATURES["mvrt_svo_combine_voxels"][1]) == 13 and len(mv.SIGNATURES["mvrt_svo_combine"][1]) == 9
    for name, value in (("UNION", 0), ("INTERSECTION", 1), ("DIFFERENCE", 2), ("XOR", 3)):
        assert "#define MVRT_COMBINE_%s %d\n" % (name, value) in src and getattr(mv, "COMBINE_" + name) == value == getattr(E, name)
    assert "#define MVRT_COMBINE_ATTRIB_B 1u\n" in src and mv.COMBINE_ATTRIB_B == E.ATTRIB_B == 1
    for name in ("combine_voxels_device", "combine_voxels", "combine"):
        assert callable(getattr(mv.IntersectorOctreeGPU, name))
    hpp = open(os.path.join(ROOT, "include", "mvrt", "IntersectorOctreeGPU.hpp")).read()
    for name in ("uint64_t combineVoxels(", "void combineVoxels(", "uint64_t combine(", "COMBINE_XOR = MVRT_COMBINE_XOR"):
        assert name in hpp


def test_refusals_that_need_no_gpu():
    """null handles, an empty handle, an unknown op or flag and an offset out of range are refused on the host, before any GPU work"""
    lib = mv.lib()
    svo = mv.IntersectorOctreeGPU()
    assert lib.mvrt_svo_combine_voxels(None, svo._h, 0, None, 0, 0, None, None, None, None, None, None, None) != 0 and b"null handle" in lib.mvrt_last_error()
    assert lib.mvrt_svo_combine(None, svo._h, 0, None, 0, None, None, None, None) != 0 and b"null handle" in lib.mvrt_last_error()
    for call in (svo.combine_voxels_device, svo.combine_voxels, svo.combine):
        with pytest.raises(mv.MvrtError, match="no octree"):
            call(svo, E.UNION)
        with pytest.raises(mv.MvrtError, match="no octree"):
            call(svo, 7, (1 << 22, 0, 0), 8)  # the handle is looked at first


def test_cpp_mirror_combine_methods_compile_and_link(tmp_path):
    exe, libdir = common.compile_usage(tmp_path, "combine_usage")
    out = subprocess.check_output([str(exe)], env=dict(os.environ, LD_LIBRARY_PATH=libdir + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", "")))
    assert b"usage" in out


def checksum(r):
    """the sum tests/cpp/combine_usage.cpp prints, modulo 2^64"""
    words = np.ascontiguousarray(r["attribs"]).view("<u4").reshape(-1, 2)
    s = 0
    for i, (v, w, src) in enumerate(zip(r["xyz"].tolist(), words.tolist(), r["source"].tolist())):
        s += (i + 1) * (v[0] + 17 * v[1] + 289 * v[2] + 4913 * src) + w[0] + 3 * w[1]
    return s % (1 << 64)


@pytest.mark.gpu
def test_cpp_mirror_agrees_with_the_python_wrapper(tmp_path):
    exe, _ = common.compile_usage(tmp_path, "combine_usage")
    out = subprocess.check_output([str(exe), "run"], timeout=120).decode()
    print(out)
    g = np.zeros((16, 16, 16), bool)
    g[2:14, 2:14, 2:14] = True
    g[3:13, 3:13, 3:13] = False
    shell = np.argwhere(g).astype(np.uint32)
    block = np.argwhere(np.ones((4, 4, 4), bool)).astype(np.uint32)
    colour = np.tile(np.array([0x10, 0x20, 0x30, 0, 0, 5, 0, 0], np.uint8), (64, 1))
    cube, brush = mv.IntersectorOctreeGPU(), mv.IntersectorOctreeGPU()
    cube.build_voxels(shell, None, gridRes=16)
    brush.build_voxels(block, colour, gridRes=4)
    offset = (9, 13, 8)
    (xa, aa), (xb, ab) = cube.read_voxels(), brush.read_voxels()
    for op in E.OPS:
        got, want = cube.combine_voxels(brush, op, offset, mv.COMBINE_ATTRIB_B), E.combine(xa, aa, xb, ab, 16, op, offset, E.ATTRIB_B)
        assert all(np.array_equal(got[k], want[k]) for k in ("xyz", "attribs", "source"))
        plain = cube.combine_voxels_device(brush, op, offset)[0]
        assert "op %d n %d sized %d overlap %d clipped %d checksum %d\n" % (op, len(got["xyz"]), plain, got["overlap"], got["clipped"], checksum(got)) in out
    assert got["overlap"] == 16 and got["clipped"] == 16
    added, removed, clipped = cube.combine(brush, E.UNION, offset)
    assert "union added %d removed %d clipped %d voxels %d emission %d\n" % (added, removed, clipped, cube.info().numberOfVoxels, cube.info().hasEmission) in out
    assert (added, removed, clipped, cube.info().hasEmission) == (32, 0, 16, 1)
    again = cube.combine(brush, E.UNION, offset)[0]
    corner = cube.combine(brush, E.DIFFERENCE)[1]
    _, carved, clipped = cube.combine(brush, E.DIFFERENCE, (9, 12, 8))
    assert "again %d corner %d carved %d clipped %d voxels %d emission %d\n" % (again, corner, carved, clipped, cube.info().numberOfVoxels, cube.info().hasEmission) in out
    assert (again, corner, carved, cube.info().hasEmission) == (0, 7, 48, 0)
