"""Exterior masks and caller-supplied face masks (mvrt_svo_surface_exterior_masks, mvrt_svo_surface_*_masked) without a GPU: the two statements of the numpy
model of tests/exterior_expected.py agree on the sets the GPU tests use, with counts pinned by hand, the bunny's counts at 64^3 with the oracle's voxelizer, the
host-side refusals of the four calls, and that every layer declares the interface."""
import ctypes as C
import os

import numpy as np
import pytest

import exterior_expected as E
import massivevoxelraytracing_amd as mv
import surface_expected as S
from common import bunny_tris
from voxel_sets import CAGE, shell, tube

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_set(res, density, seed):
    """the sets of tests/test_gpu_fill.py test_random_fill, with their six border voxels"""
    rng = np.random.default_rng(1000 * res + 10 * int(density * 10) + seed)
    xyz = np.argwhere(rng.random((res, res, res)) < density)
    border = [(0, 1, 2), (res - 1, 2, 1), (1, 0, 2), (2, res - 1, 1), (2, 1, 0), (1, 2, res - 1)]
    return np.concatenate([xyz, border])


def diagonal():
    solid = np.ones((4, 4, 3), bool)
    solid[1, 1, 1] = solid[2, 2, 1] = False
    return np.argwhere(solid)


def both_ways(xyz, res):
    """-> (voxels, faces, exterior faces, voxels with no exterior face), after E1 == E2 and the filled cells have no face"""
    v, plain, e1 = E.exterior_e1(xyz, res)
    e2, filled = E.exterior_e2(xyz, res)
    assert np.array_equal(e1, e2) and (filled == 0).all()
    assert ((e1 & ~plain) == 0).all() and (e1 < 64).all()  # bits are only ever cleared
    return len(v), E.popcount(plain), E.popcount(e1), int((e1 == 0).sum())


PINNED = [
    ("cage", lambda: CAGE, 4, (6, 36, 30, 0)),
    ("cage minus one voxel", lambda: CAGE[1:], 4, (5, 30, 30, 0)),
    ("diagonal contact", diagonal, 8, (46, 92, 80, 2)),
    ("shell on the border", lambda: shell(0, 8), 8, (296, 600, 384, 0)),
    ("nested shells", lambda: np.concatenate([shell(2, 14), shell(5, 11)]), 16, (880, 1776, 864, 152)),  # 152 = the whole inner shell
    ("tube", tube, 512, (2402, 4812, 3618, 0)),
    ("random 32 0.7 0", lambda: random_set(32, 0.7, 0), 32, (23034, 44012, 24680, 9887)),
]


@pytest.mark.parametrize("name,make,res,want", PINNED, ids=[p[0] for p in PINNED])
def test_both_statements_agree_and_counts_are_pinned(name, make, res, want):
    got = both_ways(make(), res)
    print(name, got)
    assert got == want


def test_nested_inner_shell_has_no_exterior_face():
    v, _, ext = E.exterior_e1(np.concatenate([shell(2, 14), shell(5, 11)]), 16)
    inner = ((v >= 5) & (v < 11)).all(1)
    assert inner.sum() == 152 and (ext[inner] == 0).all() and (ext[~inner] != 0).all()


def test_every_random_set_hides_faces():
    hidden = []
    for res in (16, 32):
        for density in (0.5, 0.7, 0.85):
            for seed in (0, 1):
                n, faces, ext, _ = both_ways(random_set(res, density, seed), res)
                hidden.append(faces - ext)
    print(hidden)
    assert len(hidden) == 12 and min(hidden) == 164 and max(hidden) == 19434  # none of them is vacuous


def test_bunny_at_64_with_the_oracles_voxelizer():
    from oracle import oracle as O
    O.build()
    tris = bunny_tris()
    v = tris.reshape(-1, 3)
    lo = v.min(0)
    dps = np.float32((v.max(0) - lo).max() / np.float32(64))
    xyz = S.decode(np.unique(O.voxelize(tris, lo, dps, 64, six_separating=True)[0]))
    n, faces, ext, _ = both_ways(xyz, 64)
    assert (n, faces, ext) == (8516, 27550, 14558)


def test_refusals_on_the_host():
    """a null handle, NULL masks and unknown merge flags are refused before any HIP call; an empty handle (host memory only) with "no octree" """
    lib = mv.lib()
    h = C.c_void_p(0)
    assert lib.mvrt_svo_create(C.byref(h)) == 0
    n = (C.c_uint64 * 3)(7, 7, 7)
    p = [C.byref(n, 8 * i) for i in range(3)]
    fake = C.c_void_p(64)  # a non-null masks pointer that is never read: the handle is refused first
    calls = {
        "mvrt_svo_surface_quads_masked": lambda handle, masks, flags=0: lib.mvrt_svo_surface_quads_masked(handle, masks, 0, None, None, None, p[0], None),
        "mvrt_svo_surface_mesh_masked": lambda handle, masks, flags=0: lib.mvrt_svo_surface_mesh_masked(handle, masks, 0, 0, None, None, None, None, p[0], p[1], None),
        "mvrt_svo_surface_merged_masked": lambda handle, masks, flags=0: lib.mvrt_svo_surface_merged_masked(handle, masks, flags, 0, 0, None, None, None, None, None, None, p[0], p[1],
                                                                                                             p[2], None),
    }
    try:
        for args, text in (((None, None, p[0], p[1], None), "mvrt_svo_surface_exterior_masks: null handle"),
                           ((h.value, None, p[0], p[1], None), "mvrt_svo_surface_exterior_masks: no octree")):
            assert lib.mvrt_svo_surface_exterior_masks(*args) != 0 and text in lib.mvrt_last_error().decode()
        for name, call in calls.items():
            assert call(None, fake) != 0 and name + ": null handle" in lib.mvrt_last_error().decode()
            assert call(h.value, None) != 0 and name + ": null masksDev" in lib.mvrt_last_error().decode()
            assert call(h.value, fake) != 0 and name + ": no octree" in lib.mvrt_last_error().decode()
        for flags in (4, 7, 0x80000000):
            for handle in (None, h.value):
                assert calls["mvrt_svo_surface_merged_masked"](handle, fake, flags) != 0
                assert "mvrt_svo_surface_merged_masked: unknown flags" in lib.mvrt_last_error().decode()
    finally:
        lib.mvrt_svo_destroy(h.value)
    svo = mv.IntersectorOctreeGPU()
    with pytest.raises(mv.MvrtError, match="no octree"):
        svo.surface_exterior_masks_device()
    with pytest.raises(mv.MvrtError, match="unknown flags"):
        svo.surface_merged_device(8, masks=64)


def test_header_python_and_mirror_declare_the_interface():
    src = open(os.path.join(ROOT, "include", "mvrt.h")).read()
    for name in ("mvrt_svo_surface_exterior_masks", "mvrt_svo_surface_quads_masked", "mvrt_svo_surface_mesh_masked", "mvrt_svo_surface_merged_masked"):
        assert name + "(" in src and name in mv.SIGNATURES
    assert "Stale masks" in src or "stale masks" in src  # said where callers read it
    for name in ("surface_exterior_masks_device", "surface_exterior_masks"):
        assert callable(getattr(mv.IntersectorOctreeGPU, name))
    import inspect
    for name in ("surface_quads", "surface_quads_device", "surface_mesh", "surface_mesh_device", "surface_merged", "surface_merged_device", "surface_ao"):
        par = inspect.signature(getattr(mv.IntersectorOctreeGPU, name)).parameters["masks"]
        assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is None
    hpp = open(os.path.join(ROOT, "include", "mvrt", "IntersectorOctreeGPU.hpp")).read()
    for name in ("surfaceExteriorMasks(", "surfaceQuadsMasked(", "surfaceMeshMasked(", "surfaceMergedMasked("):
        assert hpp.count(name) >= 2, name  # the device-pointer form and the host-vector form
