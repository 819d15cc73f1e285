"""The level of detail from the voxels themselves (mvrt_svo_coarse_voxels / mvrt_svo_coarsen) without a GPU: the two numpy models of tests/coarsen_expected.py
against each other and on inputs whose answer is known by hand, the bunny's counts at 128^3 with the oracle's voxelizer, the host-side refusals of the two calls
and the C++ mirror's new methods."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import common
import coarsen_expected as X
import massivevoxelraytracing_amd as mv
import surface_expected as S
from common import bunny_tris
from voxel_sets import full

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_by_hand():
    # two voxels of one cell, one of another: means round down, alpha bytes are not read and come out as 255
    xyz = [(2, 3, 0), (3, 2, 1), (5, 0, 0)]
    attribs = [(10, 20, 31, 7, 0, 1, 2, 9), (11, 21, 30, 0, 0, 2, 3, 200), (1, 2, 3, 4, 5, 6, 7, 8)]
    for model in (X.coarse, X.coarse_loop):
        got = model(xyz, attribs, 1)
        assert got["xyz"].tolist() == [[1, 1, 0], [2, 0, 0]]  # ascending Morton code: 3 and 8
        assert got["attribs"].tolist() == [[10, 20, 30, 255, 0, 1, 2, 255], [1, 2, 3, 255, 5, 6, 7, 255]] and got["count"].tolist() == [2, 1]
        assert model(xyz, attribs, 1, 2)["xyz"].tolist() == [[1, 1, 0]] and len(model(xyz, attribs, 1, 3)["xyz"]) == 0
        whole = model(xyz, attribs, 2)
        assert whole["xyz"].tolist() == [[0, 0, 0], [1, 0, 0]] and whole["count"].tolist() == [2, 1]
    for k, run in ((1, 8), (2, 64), (3, 512)):  # a full grid: aligned runs of exactly 8^k
        got = X.coarse(full(16), None, k)
        assert len(got["xyz"]) == 4096 // run and (got["count"] == run).all() and (got["attribs"] == X.default_attribs(1)).all()
        assert X.same(got, X.coarse(full(16), None, k, run)) and len(X.coarse(full(16), None, k, run)["xyz"]) == 4096 // run


def test_the_two_models_agree_on_random_sets():
    rng = np.random.default_rng(5)
    for res, density in ((4, 1.0), (8, 0.3), (8, 0.9), (16, 0.05), (16, 0.6), (32, 0.02)):
        xyz = np.argwhere(rng.random((res,) * 3) < density)
        attribs = rng.integers(0, 256, size=(len(xyz), 8), dtype=np.uint8)
        shuffled = rng.permutation(len(xyz))  # the result is a property of the set, not of its order
        levels = res.bit_length() - 1
        for k in range(1, levels):
            for min_count in (1, 2, 5, 8 ** k):
                a, b = X.coarse(xyz, attribs, k, min_count), X.coarse_loop(xyz[shuffled], attribs[shuffled], k, min_count)
                assert X.same(a, b), (res, density, k, min_count)
                codes = S.morton(a["xyz"])
                assert (np.diff(codes.astype(np.int64)) > 0).all() and (a["count"] >= min_count).all() and (a["attribs"][:, [3, 7]] == 255).all()
            assert X.coarse(xyz, attribs, k)["count"].sum() == len(xyz)


def test_levels_compose_on_the_coordinates():
    """k = a followed by k = b covers the cells of k = a + b (the attributes need not match: a mean of means differs)"""
    rng = np.random.default_rng(6)
    xyz = np.argwhere(rng.random((32,) * 3) < 0.03)
    attribs = rng.integers(0, 256, size=(len(xyz), 8), dtype=np.uint8)
    for a, b in ((1, 1), (1, 2), (2, 1), (1, 3), (2, 2)):
        first = X.coarse(xyz, attribs, a)
        second = X.coarse(first["xyz"], first["attribs"], b)
        direct = X.coarse(xyz, attribs, a + b)
        assert np.array_equal(second["xyz"], direct["xyz"])
    first = X.coarse(xyz, attribs, 1)
    assert not np.array_equal(X.coarse(first["xyz"], first["attribs"], 2)["attribs"], X.coarse(xyz, attribs, 3)["attribs"])  # (and here they do differ)


BUNNY_128 = {1: (33487, 11089, 9448), 2: (33487, 3050, 2851), 3: (33487, 769, 746)}  # k: (voxels, cells at minCount 1, cells at minCount 2)


def test_bunny_at_128_with_the_oracles_voxelizer():
    from oracle import oracle as O
    O.build()
    tris = bunny_tris()
    v = tris.reshape(-1, 3)
    lo = v.min(0)
    dps = np.float32((v.max(0) - lo).max() / np.float32(128))
    xyz = S.decode(np.unique(O.voxelize(tris, lo, dps, 128, six_separating=True)[0]))
    for k, (voxels, cells, cells2) in BUNNY_128.items():
        got, thick = X.coarse(xyz, None, k), X.coarse(xyz, None, k, 2)
        print(k, len(xyz), len(got["xyz"]), len(thick["xyz"]))
        assert (len(xyz), len(got["xyz"]), len(thick["xyz"])) == (voxels, cells, cells2)
        assert got["count"].sum() == voxels and np.array_equal(thick["xyz"], got["xyz"][got["count"] >= 2])


def test_refusals_on_the_host():
    """every refusal that the arguments or an empty handle decide, without any GPU call.  (levelsDown = log2 gridRes of a real octree: tests/test_gpu_coarsen.py)"""
    lib = mv.lib()
    h, d = C.c_void_p(0), C.c_void_p(0)
    assert lib.mvrt_svo_create(C.byref(h)) == 0 and lib.mvrt_svo_create(C.byref(d)) == 0  # host allocations only
    n = C.c_uint64(7)

    def listing(handle, k, min_count):
        return lib.mvrt_svo_coarse_voxels(handle, k, min_count, 0, None, None, None, C.byref(n), None)

    def build(src, dst, k, min_count, flags=0):
        return lib.mvrt_svo_coarsen(src, dst, k, min_count, flags, None)

    try:
        for call, who in ((lambda k, m: listing(h.value, k, m), "mvrt_svo_coarse_voxels"), (lambda k, m: build(h.value, d.value, k, m), "mvrt_svo_coarsen")):
            for k, min_count, text in ((1, 1, "no octree"), (0, 1, "levelsDown 0 is outside [1, "), (-3, 1, "levelsDown -3 is outside [1, "), (21, 1, "levelsDown 21 is outside [1, "),
                                       (1, 0, "minCount 0 is outside [1, 8^levelsDown = 8]"), (1, 9, "minCount 9 is outside [1, 8^levelsDown = 8]"),
                                       (2, 65, "minCount 65 is outside [1, 8^levelsDown = 64]"), (20, (1 << 60) + 1, "minCount 1152921504606846977 is outside [1, 8^levelsDown = 1152921504606846976]"),
                                       (20, 1 << 60, "no octree")):
                assert call(k, min_count) != 0
                assert lib.mvrt_last_error().decode().startswith(who + ": ") and text in lib.mvrt_last_error().decode(), (who, k, min_count, lib.mvrt_last_error())
        assert listing(None, 1, 1) != 0 and "mvrt_svo_coarse_voxels: null handle" in lib.mvrt_last_error().decode()
        for src, dst in ((None, d.value), (h.value, None), (None, None)):
            assert build(src, dst, 1, 1) != 0 and "mvrt_svo_coarsen: null handle" in lib.mvrt_last_error().decode()
        for flags in (4, 8, -1):
            assert build(h.value, d.value, 1, 1, flags) != 0 and "mvrt_svo_coarsen: unsupported flags" in lib.mvrt_last_error().decode()
        assert n.value == 7  # a refused listing returns no count
    finally:
        lib.mvrt_svo_destroy(h.value)
        lib.mvrt_svo_destroy(d.value)


def test_header_python_and_mirror_declare_the_interface():
    src = open(os.path.join(ROOT, "include", "mvrt.h")).read()
    for name in ("mvrt_svo_coarse_voxels", "mvrt_svo_coarsen"):
        assert name + "(" in src and name in mv.SIGNATURES
    for name in ("coarse_voxels_device", "coarse_voxels", "coarsen"):
        assert callable(getattr(mv.IntersectorOctreeGPU, name))
    hpp = open(os.path.join(ROOT, "include", "mvrt", "IntersectorOctreeGPU.hpp")).read()
    assert "coarseVoxels(" in hpp and "coarsen(" in hpp


def test_cpp_mirror_coarsen_methods_compile_and_link(tmp_path):
    exe, libdir = common.compile_usage(tmp_path, "coarsen_usage")
    out = subprocess.check_output([str(exe)], env=dict(os.environ, LD_LIBRARY_PATH=libdir + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", "")))
    assert b"usage" in out
