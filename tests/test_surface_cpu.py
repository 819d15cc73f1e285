"""The numpy model of the surface extraction (tests/surface_expected.py) against itself and against hand-checked cases, the PLY writer of
apps/scene_io.hpp through its reader, and the three layers of the interface (header, binding, C++ mirror) -- all without a GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import common
import massivevoxelraytracing_amd as mv
import surface_expected as S
from voxel_sets import DPS, LOWER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("res,n,seed", [(4, 20, 0), (8, 200, 1), (16, 700, 2), (64, 3000, 3), (256, 5000, 4)])
def test_dense_and_sparse_models_agree(res, n, seed):
    rng = np.random.default_rng(seed)
    xyz = rng.integers(0, res, size=(n, 3))
    xyz[:6] = [(0, 1, 1), (res - 1, 1, 1), (1, 0, 1), (1, res - 1, 1), (1, 1, 0), (1, 1, res - 1)]  # every grid border
    xyz = S.sorted_voxels(xyz)
    assert np.all(np.diff(S.morton(xyz).astype(np.int64)) > 0)
    a, b = S.masks_dense(xyz, res), S.masks_sparse(xyz, res)
    assert np.array_equal(a, b) and a.max() < 64 and a.min() >= 0


def test_sparse_model_at_the_21_bit_edge():
    res = 1 << 21
    xyz = S.sorted_voxels([(0, 0, 0), (res - 1, res - 1, res - 1), (res - 1, 0, 0), (res - 2, 0, 0), (5, res - 1, 7), (5, res - 1, 8)])
    m = dict(zip(map(tuple, xyz), S.masks_sparse(xyz, res)))
    assert m[(0, 0, 0)] == 63 and m[(res - 1, res - 1, res - 1)] == 63  # a 21-bit wrap would make them neighbours of each other
    assert m[(res - 1, 0, 0)] == 63 & ~(1 << 5) and m[(res - 2, 0, 0)] == 63 & ~(1 << 3)
    assert m[(5, res - 1, 7)] == 63 & ~(1 << 4) and m[(5, res - 1, 8)] == 63 & ~(1 << 2)


def test_one_voxel_by_hand():
    s = S.surface([(2, 3, 5)], 8, LOWER, DPS)
    assert s["masks"].tolist() == [63] and s["nFaces"] == 6
    assert s["faceVoxel"].tolist() == [0] * 6 and s["faceDir"].tolist() == [0, 1, 2, 3, 4, 5]
    off = [(0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1), (0, 1, 0), (1, 1, 0), (1, 1, 1), (0, 1, 1)]
    winding = [(3, 2, 1, 0), (4, 5, 6, 7), (0, 1, 5, 4), (1, 2, 6, 5), (2, 3, 7, 6), (3, 0, 4, 7)]  # -Y +Y -Z +X +Z -X
    for f in range(6):
        for k in range(4):
            c = np.array([2, 3, 5]) + off[winding[f][k]]
            want = np.array([np.float32(LOWER[a] + np.float32(np.float32(c[a]) * DPS)) for a in range(3)], np.float32)
            assert np.array_equal(s["positions"][f, k], want)
    # every face lies in the plane its direction names, on the outer side
    for f, (axis, step) in enumerate(S.DIRS):
        plane = [2, 3, 5][axis] + (1 if step > 0 else 0)
        assert np.all(s["positions"][f, :, axis] == np.float32(LOWER[axis] + np.float32(np.float32(plane) * DPS)))


def test_weld_of_one_voxel_is_eight_vertices_in_key_order():
    s = S.surface([(2, 3, 5)], 8, LOWER, DPS)
    grid = [(2 + x, 3 + y, 5 + z) for z in (0, 1) for y in (0, 1) for x in (0, 1)]  # key order: z, then y, then x
    want = np.array([[np.float32(LOWER[a] + np.float32(np.float32(c[a]) * DPS)) for a in range(3)] for c in grid], np.float32)
    assert np.array_equal(s["vertices"], want)
    assert np.array_equal(s["vertices"][s["indices"]], s["positions"])
    assert sorted(s["indices"].reshape(-1).tolist()) == sorted(list(range(8)) * 3)


@pytest.mark.parametrize("axis,plus,minus", [(0, 3, 5), (1, 1, 0), (2, 4, 2)])
def test_two_adjacent_voxels_by_hand(axis, plus, minus):
    a, b = np.array([3, 3, 3]), np.array([3, 3, 3])
    b[axis] += 1
    s = S.surface([a, b], 8, LOWER, DPS)
    assert s["nFaces"] == 10
    m = dict(zip(map(tuple, s["xyz"]), s["masks"]))
    assert m[tuple(a)] == 63 & ~(1 << plus) and m[tuple(b)] == 63 & ~(1 << minus)
    assert len(s["vertices"]) == 12  # four corners shared


def test_ply_round_trip(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "ply_check"
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "apps"), os.path.join(ROOT, "tests", "cpp", "ply_check.cpp"), "-o", str(exe)])
    rng = np.random.default_rng(9)
    s = S.surface(rng.integers(0, 16, size=(400, 3)), 16, LOWER, DPS)
    attrs = rng.integers(0, 256, size=(len(s["xyz"]), 8), dtype=np.uint8)
    for with_attrs in (True, False):
        with open(tmp_path / "in.bin", "wb") as f:
            f.write(np.array([len(s["vertices"]), s["nFaces"], len(attrs) if with_attrs else 0], np.uint64).tobytes())
            f.write(s["vertices"].tobytes() + s["indices"].tobytes() + s["faceVoxel"].tobytes() + (attrs.tobytes() if with_attrs else b""))
        subprocess.check_call([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.ply")])
        v, i, c = S.read_ply_quads(tmp_path / "out.ply")
        assert np.array_equal(v.view(np.uint32), s["vertices"].view(np.uint32)) and np.array_equal(i, s["indices"])
        assert np.array_equal(c, attrs[s["faceVoxel"], :3] if with_attrs else np.full((s["nFaces"], 3), 255, np.uint8))


def test_interface_is_declared_in_every_layer():
    header = open(os.path.join(ROOT, "include", "mvrt.h")).read()
    mirror = open(os.path.join(ROOT, "include", "mvrt", "IntersectorOctreeGPU.hpp")).read()
    for name in ("mvrt_svo_surface_masks", "mvrt_svo_surface_quads", "mvrt_svo_surface_mesh"):
        assert name + "(" in header and name in mv.SIGNATURES and name + "(" in mirror
    for name in ("surface_masks", "surface_quads", "surface_mesh"):
        assert callable(getattr(mv.IntersectorOctreeGPU, name))
    assert "lower + (float)c * dps" in header  # the position rule is stated where callers read it


def test_refusals_need_no_gpu():
    """a null handle is refused on the host before any HIP call"""
    lib = mv.lib()
    n = np.zeros(2, np.uint64)
    assert lib.mvrt_svo_surface_masks(None, None, n.ctypes.data, None) != 0 and b"null handle" in lib.mvrt_last_error()
    assert lib.mvrt_svo_surface_quads(None, 0, None, None, None, n.ctypes.data, None) != 0
    assert lib.mvrt_svo_surface_mesh(None, 0, 0, None, None, None, None, n.ctypes.data, n.ctypes.data + 8, None) != 0


def test_cpp_mirror_surface_methods_compile_and_link(tmp_path):
    exe, libdir = common.compile_usage(tmp_path, "surface_usage")
    out = subprocess.check_output([str(exe)], env=dict(os.environ, LD_LIBRARY_PATH=libdir + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", "")))
    assert b"usage" in out
