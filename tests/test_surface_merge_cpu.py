"""The numpy model of the merged surface (tests/merge_expected.py) against an independent brute force and hand-checked cases, the two invariants of the rule
(include/mvrt.h, mvrt_svo_surface_merged) on every case, and the layers of the interface (header, binding, C++ mirror) -- all without a GPU."""
import os
import subprocess

import numpy as np
import pytest

import common
import massivevoxelraytracing_amd as mv
import merge_expected as M
import surface_expected as S
from voxel_sets import DPS, LOWER, full

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute_force(xyz, attrs, res, any_attribute):
    """per direction and plane a dense 2-D image of the faces and their attributes, walked with plain loops -> [(d, p, u0, v0, du, dv, vIndex)] in order"""
    index = {tuple(p): i for i, p in enumerate(xyz.tolist())}
    rects = []
    for d, (axis, step) in enumerate(S.DIRS):
        ua, va = M.UV_AXES[axis]
        for p in range(res):
            face = np.zeros((res, res), bool)
            attr = np.zeros((res, res), np.uint64)
            vox = np.zeros((res, res), np.int64)
            for c, i in index.items():
                n = list(c)
                n[axis] += step
                if c[axis] == p and tuple(n) not in index:  # outside the grid is not in the set either
                    face[c[ua], c[va]] = True
                    attr[c[ua], c[va]] = 0 if any_attribute else int(attrs[i].view(np.uint64)[0])
                    vox[c[ua], c[va]] = i
            runs = {}  # (u0, v) -> du
            for v in range(res):
                u = 0
                while u < res:
                    if not face[u, v]:
                        u += 1
                        continue
                    u0 = u
                    while u + 1 < res and face[u + 1, v] and attr[u + 1, v] == attr[u, v]:
                        u += 1
                    runs[(u0, v)] = u - u0 + 1
                    u += 1
            for (u0, v0) in sorted(runs):
                below = (u0, v0 - 1)
                if below in runs and runs[below] == runs[(u0, v0)] and attr[u0, v0 - 1] == attr[u0, v0]:
                    continue  # not the first of its stack
                v = v0
                while (u0, v + 1) in runs and runs[(u0, v + 1)] == runs[(u0, v0)] and attr[u0, v + 1] == attr[u0, v]:
                    v += 1
                rects.append((d, p, u0, v0, runs[(u0, v0)], v - v0 + 1, int(vox[u0, v0])))
    return rects


def model(xyz, res, attrs=None, flags=0):
    xyz = S.sorted_voxels(xyz)
    m = M.merged(xyz, attrs, res, LOWER, DPS, flags)
    check_invariants(xyz, res, m)
    return xyz, m


def check_invariants(xyz, res, m):
    masks = S.masks_of(xyz, res)
    assert int(m["rectSize"].astype(np.int64).prod(1).sum()) == m["nFaces"] == S.surface(xyz, res, LOWER, DPS)["nFaces"]
    assert M.same_face_set(M.rasterise(xyz, m["rectVoxel"], m["rectDir"], m["rectSize"]), M.face_rows(xyz, masks))


def as_tuples(xyz, m):
    out = []
    for vox, d, (du, dv) in zip(m["rectVoxel"].tolist(), m["rectDir"].tolist(), m["rectSize"].tolist()):
        axis = S.DIRS[d][0]
        ua, va = M.UV_AXES[axis]
        out.append((d, int(xyz[vox][axis]), int(xyz[vox][ua]), int(xyz[vox][va]), du, dv, vox))
    return out


L_SHAPE = [(0, 0, 0), (1, 0, 0), (2, 0, 0), (0, 0, 1), (1, 0, 1)]


@pytest.mark.parametrize("any_attribute", [False, True])
@pytest.mark.parametrize("palette", [1, 2, 3])
@pytest.mark.parametrize("res,density", [(4, 0.5), (8, 0.3), (8, 0.8), (16, 0.6)])
def test_model_against_brute_force(res, density, palette, any_attribute):
    rng = np.random.default_rng(100 * res + 10 * palette + int(any_attribute))
    xyz = S.sorted_voxels(np.argwhere(rng.random((res, res, res)) < density))
    colours = rng.integers(0, 256, size=(palette, 8), dtype=np.uint8)
    attrs = colours[rng.integers(0, palette, size=len(xyz))]
    _, m = model(xyz, res, attrs, M.ANY_ATTRIBUTE if any_attribute else 0)
    want = brute_force(xyz, attrs, res, any_attribute)
    assert as_tuples(xyz, m) == want
    assert want == sorted(want, key=lambda r: r[:4])  # ascending (d, p, u0, v0)
    if palette == 1:  # one attribute value: the flag changes nothing
        assert as_tuples(xyz, M.merged(xyz, attrs, res, LOWER, DPS, M.ANY_ATTRIBUTE)) == want


def test_one_voxel_by_hand():
    xyz, m = model([(2, 3, 5)], 8, flags=M.WELD)
    s = S.surface([(2, 3, 5)], 8, LOWER, DPS)
    assert m["rectVoxel"].tolist() == s["faceVoxel"].tolist() and m["rectDir"].tolist() == s["faceDir"].tolist() and m["rectSize"].tolist() == [[1, 1]] * 6
    assert np.array_equal(m["positions"].view(np.uint32), s["positions"].view(np.uint32))
    assert np.array_equal(m["vertices"].view(np.uint32), s["vertices"].view(np.uint32)) and np.array_equal(m["indices"], s["indices"])


@pytest.mark.parametrize("res", [2, 4, 8])
def test_full_grid_is_six_squares(res):
    xyz, m = model(full(res), res, flags=M.WELD)
    assert m["rectDir"].tolist() == [0, 1, 2, 3, 4, 5] and m["rectSize"].tolist() == [[res, res]] * 6
    assert len(m["vertices"]) == 8 and sorted(m["indices"].reshape(-1).tolist()) == sorted(list(range(8)) * 3)
    lo, hi = LOWER, (LOWER + np.float32(res) * DPS).astype(np.float32)
    assert np.array_equal(m["vertices"][0], lo) and np.array_equal(m["vertices"][7], hi)
    s = S.surface(full(res), res, LOWER, DPS)  # the same winding as the unmerged face of the anchor voxel: corner k lies on the same side of the centre
    for r in range(6):
        f = np.nonzero((s["faceVoxel"] == m["rectVoxel"][r]) & (s["faceDir"] == r))[0][0]
        assert np.array_equal(np.sign(m["positions"][r] - m["positions"][r].mean(0)), np.sign(s["positions"][f] - s["positions"][f].mean(0)))


def test_the_L_gives_ten_rectangles():
    """Five voxels in the plane y = 0, rows x = 0..2 at z = 0 and x = 0..1 at z = 1: 5 faces each on -Y and +Y and an outline of 10 edges, 20 faces (what
    mvrt_svo_surface_masks counts), in 10 rectangles.  The two -X caps lie at consecutive v = z in one column and stack into a 1 x 2."""
    xyz, m = model(L_SHAPE, 4)
    assert m["nFaces"] == 20 and len(m["rectVoxel"]) == 10
    by_dir = {d: sorted(map(tuple, m["rectSize"][m["rectDir"] == d].tolist())) for d in range(6)}
    assert by_dir[0] == by_dir[1] == [(2, 1), (3, 1)]  # -Y, +Y: (u, v) = (x, z); rows of 3 and 2 do not stack
    assert by_dir[2] == [(3, 1)] and by_dir[4] == [(1, 1), (2, 1)]  # -Z: the whole z = 0 row; +Z: (2,0,0) alone, and the z = 1 row
    assert by_dir[5] == [(1, 2)] and by_dir[3] == [(1, 1), (1, 1)]  # -X: (u, v) = (y, z), one 1 x 2 stack; +X: (2,0,0) and (1,0,1) lie in different planes
    sizes = sorted(map(tuple, m["rectSize"].tolist()))
    assert sizes.count((3, 1)) == 3 and sizes.count((2, 1)) == 3 and sizes.count((1, 1)) == 3 and sizes.count((1, 2)) == 1


@pytest.mark.parametrize("res", [4, 1 << 21])
def test_row_wrap_pair_stays_unmerged(res):
    """for +Y, (u, v) = (x, z): the last face of row v and the first of row v + 1 are neighbours in a packed key, not in the grid"""
    y, z = (1, 1) if res == 4 else (5, 7)
    xyz, m = model([(res - 1, y, z), (0, y, z + 1)], res)
    assert m["nFaces"] == 12 and len(m["rectVoxel"]) == 12 and m["rectSize"].tolist() == [[1, 1]] * 12
    # the same trap in step 2, where v is the low field: for +-X (u, v) = (y, z), so columns u = y and u = y + 1 meet at z = res - 1 | 0
    xyz, m = model([(2, y, res - 1), (2, y + 1, 0)], res)
    assert len(m["rectVoxel"]) == 12


@pytest.mark.parametrize("res", [16, 1 << 21])
def test_pair_at_the_upper_edge_merges(res):
    xyz, m = model([(res - 2, 9, 9), (res - 1, 9, 9)], res)
    assert m["nFaces"] == 10 and len(m["rectVoxel"]) == 6
    assert [tuple(s) for s in m["rectSize"].tolist()] == [(2, 1), (2, 1), (2, 1), (1, 1), (2, 1), (1, 1)]  # -Y +Y -Z +X +Z -X
    assert m["rectVoxel"].tolist() == [0, 0, 0, 1, 0, 0]


def test_attributes_split_and_the_flag_joins():
    xyz = S.sorted_voxels([(x, 0, 0) for x in range(4)])
    attrs = np.zeros((4, 8), np.uint8)
    attrs[2:, 7] = 1  # the last byte alone
    _, m = model(xyz, 4, attrs)
    assert len(m["rectVoxel"]) == 2 + 4 * 2
    _, m = model(xyz, 4, attrs, M.ANY_ATTRIBUTE)
    assert len(m["rectVoxel"]) == 6


def test_interface_is_declared_in_every_layer():
    header = open(os.path.join(ROOT, "include", "mvrt.h")).read()
    mirror = open(os.path.join(ROOT, "include", "mvrt", "IntersectorOctreeGPU.hpp")).read()
    assert "mvrt_svo_surface_merged(" in header and "mvrt_svo_surface_merged" in mv.SIGNATURES and "mvrt_svo_surface_merged(" in mirror
    assert mirror.count("surfaceMerged(") >= 3  # both forms and a call
    assert callable(mv.IntersectorOctreeGPU.surface_merged) and callable(mv.IntersectorOctreeGPU.surface_merged_device)
    assert (mv.SURFACE_MERGE_ANY_ATTRIBUTE, mv.SURFACE_MERGE_WELD) == (1, 2) == (M.ANY_ATTRIBUTE, M.WELD)
    assert "#define MVRT_SURFACE_MERGE_ANY_ATTRIBUTE 1" in header and "#define MVRT_SURFACE_MERGE_WELD 2" in header
    assert "T-junctions" in header  # said where callers read it


def test_refusals_need_no_gpu():
    """a null handle and unknown flag bits are refused on the host before any HIP call"""
    lib = mv.lib()
    n = np.zeros(3, np.uint64)

    def call(handle, flags, indices=None):
        return lib.mvrt_svo_surface_merged(handle, flags, 0, 0, None, None, None, None, indices, None, n.ctypes.data, n.ctypes.data + 8, n.ctypes.data + 16, None)

    for flags in (0, 1, 2, 3):
        assert call(None, flags) != 0 and b"null handle" in lib.mvrt_last_error()
    for flags in (4, 7, 0x80000000):
        assert call(None, flags) != 0 and b"unknown flags" in lib.mvrt_last_error()
    # an empty handle (mvrt_svo_create only allocates host memory): "no octree", and the flags are looked at all the same
    svo = mv.IntersectorOctreeGPU()
    with pytest.raises(mv.MvrtError, match="no octree"):
        svo.surface_merged_device(3)
    with pytest.raises(mv.MvrtError, match="unknown flags"):
        svo.surface_merged_device(8)


def test_cpp_mirror_merge_methods_compile_and_link(tmp_path):
    exe, libdir = common.compile_usage(tmp_path, "surface_merge_usage")
    out = subprocess.check_output([str(exe)], env=dict(os.environ, LD_LIBRARY_PATH=libdir + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", "")))
    assert b"usage" in out
