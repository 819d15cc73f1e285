"""The nearest-voxel query interface: the header, the Python table and the C++ mirror declare the calls, and tests/cpp/query_usage.cpp, which pins their C
signatures, compiles and links against the library -- without a GPU, where it also checks the refusals the host makes before any GPU work.  On a GPU the program
is run, and every line it prints is compared with what the Python wrapper and the model of tests/query_expected.py give for the same sets."""
import os
import subprocess

import numpy as np
import pytest

import common
import massivevoxelraytracing_amd as mv
import query_expected as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("mvrt_svo_nearest_voxels", "mvrt_svo_nearest_between", "mvrt_svo_transfer_attributes", "mvrt_test_nearest_query_stats")
M64 = (1 << 64) - 1


def test_header_python_and_mirror_declare_the_interface():
    src = open(os.path.join(ROOT, "include", "mvrt.h")).read()
    for name in CALLS:
        assert name + "(" in src and name in mv.SIGNATURES
    assert [len(mv.SIGNATURES[n][1]) for n in CALLS] == [8, 13, 8, 1]
    for fact in ("d2 is below 2^47 and is a uint64 everywhere", "UINT64_MAX means no limit, 0 is legal and is the membership test", "the limit never changes an answer that lies within it",
                 "STRICTLY further", "near is taken in src BEFORE anything is written", "nOverlap of mvrt_svo_combine_voxels on equal grids", "both NULL is the summary call",
                 "#define MVRT_TRANSFER_COLOUR 1u", "#define MVRT_TRANSFER_EMISSION 2u", "n >= 2^32 is refused", "each in [-2^22, 2^22]"):
        assert fact in src, fact  # the facts that pin the conventions are stated in the header
    for name in ("nearest_voxels_device", "nearest_voxels", "nearest_between_device", "nearest_between", "transfer_attributes"):
        assert callable(getattr(mv.IntersectorOctreeGPU, name))
    assert callable(mv.nearest_query_stats) and (mv.TRANSFER_COLOUR, mv.TRANSFER_EMISSION, mv.NO_LIMIT) == (1, 2, M64)
    hpp = open(os.path.join(ROOT, "include", "mvrt", "IntersectorOctreeGPU.hpp")).read()
    assert hpp.count("void nearestVoxels(") == 2 and hpp.count("Between nearestBetween(") == 2 and "uint64_t transferAttributes(" in hpp


def test_refusals_that_need_no_gpu():
    svo = mv.IntersectorOctreeGPU()
    allocs = mv.allocation_state()[2]
    q = np.zeros((3, 3), np.int32)
    for call in (lambda: svo.nearest_voxels_device(3, 8), lambda: svo.nearest_voxels(q), lambda: svo.nearest_between_device(svo), lambda: svo.nearest_between(svo),
                 lambda: svo.transfer_attributes(svo)):
        with pytest.raises(mv.MvrtError, match="no octree"):
            call()
    with pytest.raises(ValueError, match="outside"):
        svo.nearest_voxels(np.array([(0, (1 << 22) + 1, 0)], np.int32))
    assert mv.allocation_state()[2] == allocs  # no device allocation was attempted
    assert set(mv.nearest_query_stats()) == {"queries", "visits", "most", "compared"}  # (a refusal on the host leaves the figures of the call before)


def test_cpp_mirror_query_methods_compile_link_and_refuse(tmp_path):
    exe, libdir = common.compile_usage(tmp_path, "query_usage")
    r = subprocess.run([str(exe)], env=dict(os.environ, LD_LIBRARY_PATH=libdir + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", "")), capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "usage" in r.stdout and "(0 host checks failed)" in r.stdout


def shell(o, tint):
    """the set of tests/cpp/query_usage.cpp"""
    cube = np.array([(x, y, z) for z in range(7) for y in range(7) for x in range(7) if x % 6 == 0 or y % 6 == 0 or z % 6 == 0], np.uint32)
    colour = np.zeros((len(cube), 2), "<u4")
    colour[:, 0] = 0x21 * cube[:, 0] + 0x2000 * cube[:, 1] + 0x200000 * cube[:, 2] + tint
    colour[cube[:, 0] == 0, 1] = 0x700
    return cube + o, colour.view(np.uint8).reshape(-1, 8)


def checksum(dist2, nearest, attribs=None):
    """the sums tests/cpp/query_usage.cpp prints, modulo 2^64"""
    words = None if attribs is None else np.ascontiguousarray(attribs).view("<u4").reshape(-1, 2).tolist()
    s = 0
    for i, (d, v) in enumerate(zip(dist2.tolist(), nearest.tolist())):
        s += (i + 1) * (d + 4913 * v) + (words[i][0] + 3 * words[i][1] if words else 0)
    return s & M64


@pytest.mark.gpu
def test_cpp_mirror_agrees_with_the_python_wrapper_and_the_model(tmp_path):
    exe, _ = common.compile_usage(tmp_path, "query_usage")
    out = subprocess.check_output([str(exe), "run"], timeout=120).decode()
    print(out)
    (xa, ca), (xb, cb) = shell(4, 0), shell(6, 0x010101)
    a, b = mv.IntersectorOctreeGPU(), mv.IntersectorOctreeGPU()
    a.build_voxels(xa, ca, dps=1.0 / 16, gridRes=16)
    b.build_voxels(xb, cb, dps=1.0 / 16, gridRes=16)
    q = np.array([(x, y, z) for z in range(16) for y in range(16) for x in range(16)] + [(x, y, z) for x in (-9, 3, 24) for y in (-1, 16) for z in (-17, 40)], np.int32)
    xa0, ca0 = a.read_voxels()
    for limit, line in ((Q.NO_LIMIT, "queries %d checksum %%d\n" % len(q)), (9, "limit 9 checksum %d\n")):
        got, want = a.nearest_voxels(q, limit), Q.nearest_voxels(xa0, ca0, q, limit)
        assert all(np.array_equal(got[k], want[k]) for k in ("dist2", "nearest", "attribs"))
        assert line % checksum(want["dist2"], want["nearest"], want["attribs"]) in out
    o = (1, 0, -1)
    got, want, lim = a.nearest_between(b, o), Q.nearest_between(xa, xb, o), Q.nearest_between(xa, xb, o, 4)
    assert all(got[k] == want[k] for k in ("n", "maxDist2", "farthest", "zero", "beyond")) and np.array_equal(got["dist2"], want["dist2"]) and np.array_equal(got["nearest"], want["nearest"])
    assert "between n %d max %d farthest %d zero %d beyond %d checksum %d; limit 4: max %d farthest %d beyond %d\n" % (
        want["n"], want["maxDist2"], want["farthest"], want["zero"], want["beyond"], checksum(want["dist2"], want["nearest"]), lim["maxDist2"], lim["farthest"], lim["beyond"]) in out
    assert 0 < lim["beyond"] < want["n"]
    _, new, taken, changed = Q.transferred(xa0, ca0, *b.read_voxels(), o, 4, mv.TRANSFER_COLOUR)
    assert a.transfer_attributes(b, o, 4, mv.TRANSFER_COLOUR) == (changed, int((~taken).sum())) and np.array_equal(a.read_voxels()[1], new)
    words = new.view("<u4").reshape(-1, 2).tolist()
    total = sum((i + 1) * (w[0] + 3 * w[1]) for i, w in enumerate(words)) & M64
    assert "transfer changed %d beyond %d again 0 emission 1 checksum %d\n" % (changed, int((~taken).sum()), total) in out
