"""Enclosed empty cells and the fill (mvrt_svo_enclosed_cells / mvrt_svo_fill_enclosed) without a GPU: the numpy model of tests/fill_expected.py on inputs whose
answer is known by hand, against scipy's labelling where scipy is installed, the bunny's counts at 64^3 with the oracle's voxelizer, the host-side refusals of
the two calls, and the C++ mirror's new methods."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import common
import fill_expected as F
import massivevoxelraytracing_amd as mv
import surface_expected as S
from common import bunny_tris
from voxel_sets import CAGE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cage_of_six_voxels():
    want = F.enclosed(CAGE, 4)
    assert want["xyz"].tolist() == [[1, 1, 1]] and want["region"].tolist() == [0] and want["nRegions"] == 1
    for gone in range(6):
        open_cage = F.enclosed(CAGE[:gone] + CAGE[gone + 1:], 4)
        assert len(open_cage["xyz"]) == 0 and len(open_cage["region"]) == 0 and open_cage["nRegions"] == 0


def test_diagonal_contact_does_not_connect_and_regions_number_by_first_morton_appearance():
    # two one-cell cavities at (1, 1, 1) and (2, 2, 1) touch along an edge only; everything else of the 4 x 4 x 3 slab [0, 4) x [0, 4) x [0, 3) is solid
    solid = np.ones((4, 4, 3), bool)
    solid[1, 1, 1] = solid[2, 2, 1] = False
    want = F.enclosed(np.argwhere(solid), 8)
    assert want["xyz"].tolist() == [[1, 1, 1], [2, 2, 1]] and want["region"].tolist() == [0, 1] and want["nRegions"] == 2
    # a shell that touches the grid border still encloses its inside
    g = np.ones((8, 8, 8), bool)
    g[1:7, 1:7, 1:7] = False
    shell = F.enclosed(np.argwhere(g), 8)
    assert len(shell["xyz"]) == 216 and shell["nRegions"] == 1 and not shell["region"].any()
    assert np.array_equal(S.morton(shell["xyz"]), np.sort(S.morton(shell["xyz"])))


def test_model_equals_scipy_labelling():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(3)
    seen = 0
    for res, density in [(8, 0.5), (8, 0.7), (16, 0.5), (16, 0.7), (16, 0.85), (32, 0.7)]:
        solid = rng.random((res,) * 3) < density
        label, n = ndimage.label(~solid)  # 6-connectivity is scipy's default structure
        border = np.ones_like(solid)
        border[1:-1, 1:-1, 1:-1] = False
        outside = np.unique(label[border & ~solid])
        inside = ~solid & ~np.isin(label, outside)
        cells = np.argwhere(inside)
        cells = cells[np.argsort(S.morton(cells), kind="stable")]
        labels = label[cells[:, 0], cells[:, 1], cells[:, 2]]
        _, first = np.unique(labels, return_index=True)
        rank = {labels[i]: k for k, i in enumerate(np.sort(first))}
        want = F.enclosed(np.argwhere(solid), res)
        assert np.array_equal(want["xyz"], cells) and want["region"].tolist() == [rank[l] for l in labels] and want["nRegions"] == len(first)
        seen += len(cells)
    assert seen > 50


def test_bunny_at_64_with_the_oracles_voxelizer():
    from oracle import oracle as O
    O.build()
    tris = bunny_tris()
    v = tris.reshape(-1, 3)
    lo = v.min(0)
    dps = np.float32((v.max(0) - lo).max() / np.float32(64))
    for six, voxels, cells, sizes in ((True, 8516, 48162, [48159, 2, 1]), (False, 13774, 45658, None)):
        codes = np.unique(O.voxelize(tris, lo, dps, 64, six_separating=six)[0])
        xyz = S.decode(codes)
        want = F.enclosed(xyz, 64)
        assert len(codes) == voxels and len(want["xyz"]) == cells
        if sizes:
            assert want["nRegions"] == 3 and sorted(np.bincount(want["region"]).tolist(), reverse=True) == sizes
            # what the fill saves the mesh export: the inner side of the shell
            assert S.surface(xyz, 64, lo, dps)["nFaces"] == 27550 and S.surface(F.filled_set(xyz, 64), 64, lo, dps)["nFaces"] == 14558


def test_refusals_on_the_host():
    lib = mv.lib()
    h = C.c_void_p(0)
    assert lib.mvrt_svo_create(C.byref(h)) == 0  # host allocation only
    nc, nr = C.c_uint64(7), C.c_uint64(7)
    try:
        for args, text in (((None, 0, None, None, C.byref(nc), C.byref(nr), None), "mvrt_svo_enclosed_cells: null handle"),
                           ((h.value, 0, None, None, C.byref(nc), C.byref(nr), None), "mvrt_svo_enclosed_cells: no octree")):
            assert lib.mvrt_svo_enclosed_cells(*args) != 0 and text in lib.mvrt_last_error().decode()
        for args, text in (((None, None, C.byref(nc), None), "mvrt_svo_fill_enclosed: null handle"), ((h.value, None, C.byref(nc), None), "mvrt_svo_fill_enclosed: no octree")):
            assert lib.mvrt_svo_fill_enclosed(*args) != 0 and text in lib.mvrt_last_error().decode()
    finally:
        lib.mvrt_svo_destroy(h.value)


def test_header_python_and_mirror_declare_the_interface():
    src = open(os.path.join(ROOT, "include", "mvrt.h")).read()
    for name in ("mvrt_svo_enclosed_cells", "mvrt_svo_fill_enclosed"):
        assert name + "(" in src and name in mv.SIGNATURES
    for name in ("enclosed_cells_device", "enclosed_cells", "fill_enclosed"):
        assert callable(getattr(mv.IntersectorOctreeGPU, name))
    hpp = open(os.path.join(ROOT, "include", "mvrt", "IntersectorOctreeGPU.hpp")).read()
    assert "enclosedCells(" in hpp and "fillEnclosed(" in hpp


def test_cpp_mirror_fill_methods_compile_and_link(tmp_path):
    exe, libdir = common.compile_usage(tmp_path, "fill_usage")
    out = subprocess.check_output([str(exe)], env=dict(os.environ, LD_LIBRARY_PATH=libdir + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", "")))
    assert b"usage" in out
