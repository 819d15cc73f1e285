"""The nearest-voxel interface of the enclosed cells: the header, the Python table and the C++ mirror declare the calls, and tests/cpp/nearest_usage.cpp, which pins
their C signatures, compiles and links against the library -- without a GPU, where it also checks the refusals the host makes before any GPU work.  On a GPU the
program is run, and every line it prints is compared with what the Python wrapper and the model of tests/nearest_expected.py give for the same set."""
import os
import subprocess

import numpy as np
import pytest

import common
import massivevoxelraytracing_amd as mv
import nearest_expected as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("mvrt_svo_enclosed_nearest", "mvrt_svo_fill_enclosed_nearest", "mvrt_test_enclosed_nearest_stats")


def test_header_python_and_mirror_declare_the_interface():
    src = open(os.path.join(ROOT, "include", "mvrt.h")).read()
    for name in CALLS:
        assert name + "(" in src and name in mv.SIGNATURES
    assert [len(mv.SIGNATURES[n][1]) for n in CALLS] == [10, 3, 1]
    for fact in ("dist2 < 2^20 always", "near(c) is taken on the set BEFORE the fill", "A shell with emission makes emissive","there is no radius"):
        assert fact in src  # the facts that pin the conventions are stated in the header
    for name in ("enclosed_nearest_device", "enclosed_nearest", "fill_enclosed_nearest"):
        assert callable(getattr(mv.IntersectorOctreeGPU, name))
    assert callable(mv.enclosed_nearest_stats)
    hpp = open(os.path.join(ROOT, "include", "mvrt", "IntersectorOctreeGPU.hpp")).read()
    assert hpp.count("uint64_t enclosedNearest(") == 2 and "uint64_t fillEnclosedNearest(" in hpp


def test_refusals_that_need_no_gpu():
    svo = mv.IntersectorOctreeGPU()
    allocs = mv.allocation_state()[2]
    for call in (svo.enclosed_nearest_device, svo.enclosed_nearest, svo.fill_enclosed_nearest):
        with pytest.raises(mv.MvrtError, match="no octree"):
            call()
    assert mv.allocation_state()[2] == allocs  # no device allocation was attempted
    assert mv.enclosed_nearest_stats() == {"cells": 0, "gaps": [0, 0, 0], "longest": [0, 0, 0], "deepest": 0}


def test_cpp_mirror_nearest_methods_compile_link_and_refuse(tmp_path):
    exe, libdir = common.compile_usage(tmp_path, "nearest_usage")
    r = subprocess.run([str(exe)], env=dict(os.environ, LD_LIBRARY_PATH=libdir + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", "")), capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "usage" in r.stdout and "(0 host checks failed)" in r.stdout


def checksum(r):
    """the sum tests/cpp/nearest_usage.cpp prints, modulo 2^64"""
    words = np.ascontiguousarray(r["attribs"]).view("<u4").reshape(-1, 2)
    s = 0
    for i, (v, d, near, reg, w) in enumerate(zip(r["xyz"].tolist(), r["dist2"].tolist(), r["nearest"].tolist(), r["region"].tolist(), words.tolist())):
        s += (i + 1) * (v[0] + 17 * v[1] + 289 * v[2] + 4913 * d + 83521 * near + reg) + w[0] + 3 * w[1]
    return s % (1 << 64)


@pytest.mark.gpu
def test_cpp_mirror_agrees_with_the_python_wrapper_and_the_model(tmp_path):
    exe, _ = common.compile_usage(tmp_path, "nearest_usage")
    out = subprocess.check_output([str(exe), "run"], timeout=120).decode()
    print(out)
    cube = np.array([(x, y, z) for z in range(7) for y in range(7) for x in range(7) if x % 6 == 0 or y % 6 == 0 or z % 6 == 0 or (x, y, z) == (2, 4, 3)], np.uint32)
    colour = np.zeros((len(cube), 2), "<u4")
    colour[:, 0] = 0x21 * cube[:, 0] + 0x2000 * cube[:, 1] + 0x200000 * cube[:, 2]
    colour[cube[:, 0] == 0, 1] = 0x700
    svo = mv.IntersectorOctreeGPU()
    svo.build_voxels(cube + 2, colour.view(np.uint8).reshape(-1, 8), dps=1.0 / 16, gridRes=16)
    x0, a0 = svo.read_voxels()
    got, want = svo.enclosed_nearest(), N.enclosed_nearest(x0, a0, 16)
    assert all(np.array_equal(got[k], want[k]) for k in ("xyz", "region", "dist2", "nearest", "attribs")) and len(want["xyz"]) == 124
    assert "listing n 124 sized 124 regions 1 1 deepest %d checksum %d\n" % (want["dist2"].max(), checksum(want)) in out
    assert svo.fill_enclosed_nearest() == 124
    assert "fill voxels %d -> %d filled 124 again 0 emission 1\n" % (len(x0), svo.info().numberOfVoxels) in out
