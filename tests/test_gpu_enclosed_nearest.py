"""The nearest voxel of every enclosed cell and the fill with its colours on the GPU (mvrt_svo_enclosed_nearest / mvrt_svo_fill_enclosed_nearest)
against the numpy model of tests/nearest_expected.py, which takes the minimum over all voxels by brute force and knows nothing of the three passes: xyz, region,
dist2, nearest and attribs bit for bit, on the smallest shapes that can break each mechanism -- one cell with six ties, the cage whose ties arrive in three
passes, debris that makes the nearest voxel differ in all three axes, tubes along every axis at the wave and workgroup seams of the run expansion, thousands of
short gaps, mass ties in a sphere, cavities behind a one-voxel wall, nesting, the far corner of the 2^21 grid, a one-cell corridor -- then the agreement with the
band engine of mvrt_svo_distance_cells, the contract of the listing, and the fill against an edit with the model's cells."""
import ctypes as C
import os

import numpy as np
import pytest

import ball_expected as B
import nearest_expected as N
import surface_expected as S
from common import GOLDEN, bunny_tris, probe_camera
from fixtures import mv  # noqa: F401 (fixtures)
from voxel_sets import DPS, LOWER, assert_same_octree, colours, filled, full, octree, same, serpentine, shell

pytestmark = pytest.mark.gpu

KEYS = ("xyz", "region", "dist2", "nearest", "attribs")


def build(mv, xyz, res, flags=0, attribs=None, emission=True):
    xyz = np.ascontiguousarray(xyz, np.uint32).reshape(-1, 3)
    svo = mv.IntersectorOctreeGPU()
    svo.build_voxels(xyz, colours(len(xyz), emission=emission) if attribs is None else attribs, origin=LOWER, dps=DPS, gridRes=res, flags=flags)
    return svo


def assert_listing(svo, res, want=None):
    """the listing of the handle against the model on the voxels the handle holds; -> the model's listing"""
    if want is None:
        x0, a0 = svo.read_voxels()
        want = N.enclosed_nearest(x0, a0, res)
    n = len(want["xyz"])
    assert svo.enclosed_nearest_device() == (n, want["nRegions"])  # the sizing call
    got = svo.enclosed_nearest()
    print("cells", len(got["xyz"]), "regions", got["nRegions"], "model", n, want["nRegions"], "deepest", int(want["dist2"].max()) if n else 0)
    assert got["nRegions"] == want["nRegions"]
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    return want


def check(mv, xyz, res, flags=0, attribs=None):
    svo = build(mv, xyz, res, flags, attribs)
    return svo, assert_listing(svo, res)


def open_cage():
    """the shell around a 3^3 cavity with the centre of one face missing: nothing is enclosed"""
    c = shell(1, 6)
    return c[~(c == (3, 3, 1)).all(1)]


def debris_cavity(res=32, size=24, percent=3, seed=5):
    """a cavity of size^3 cells in a one-voxel shell, with `percent` % of its cells made voxels"""
    lo = (res - size) // 2 - 1
    inner = full(size) + lo + 1
    keep = np.random.default_rng(seed).random(len(inner)) * 100 < percent
    return np.concatenate([shell(lo, lo + size + 2), inner[keep]])


# ---- ties, passes, seams ---------------------------------------------------------------------------------------------------------------------------------------
def test_one_cell_with_six_ties_at_coordinate_zero(mv):
    _, want = check(mv, shell(0, 3), 4)
    assert want["xyz"].tolist() == [[1, 1, 1]] and want["dist2"].tolist() == [1]
    assert want["nearest"].tolist() == [3]  # (1, 1, 0), code 3, is the lowest of the six in Morton order, behind the voxels with the codes 0, 1 and 2


def test_cage_ties_arrive_in_three_passes(mv):
    svo, want = check(mv, shell(1, 6), 8)
    d2 = {tuple(c): int(d) for c, d in zip(want["xyz"].tolist(), want["dist2"])}
    assert len(d2) == 27 and d2[(3, 3, 3)] == 4 and all(d2[c] == 1 for c in [(2, 2, 2), (4, 2, 2), (2, 4, 4), (4, 4, 4)])
    stats = mv.enclosed_nearest_stats()
    assert stats == {"cells": 27, "gaps": [9, 9, 9], "longest": [3, 3, 3], "deepest": 4}
    assert svo.enclosed_nearest_device() == (27, 1) and mv.enclosed_nearest_stats() == {"cells": 27, "gaps": [0] * 3, "longest": [0] * 3, "deepest": 0}  # the sizing call


def test_a_floating_voxel_is_nearest_across_all_three_axes(mv):
    xyz = np.concatenate([shell(2, 13), [(6, 8, 5)]])  # a cavity of 9^3
    _, want = check(mv, xyz, 16)
    x0 = xyz[np.argsort(S.morton(xyz), kind="stable")]
    off = want["xyz"].astype(np.int64) - x0[want["nearest"]]
    assert ((off != 0).all(1) & (x0[want["nearest"]] == (6, 8, 5)).all(1)).sum() > 20


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("length", [63, 64, 65, 255, 256, 257])
def test_tubes_across_the_seams(mv, axis, length):
    """5 x 5 x L cells through a block, one debris voxel inside, off centre"""
    hi = [9, 9, 9]
    hi[axis] = length + 4
    at = [4, 5, 3]
    at[axis] = 2 + length // 3
    svo, want = check(mv, np.concatenate([shell((2, 2, 2), hi), [at]]), 512)
    assert len(want["xyz"]) == 25 * length - 1
    assert mv.enclosed_nearest_stats()["longest"][axis] == length


def test_thousands_of_short_gaps(mv):
    svo, want = check(mv, debris_cavity(), 32)
    stats = mv.enclosed_nearest_stats()
    print(stats)
    assert stats["cells"] == len(want["xyz"]) and min(stats["gaps"]) > 256 * 3 and stats["deepest"] == want["dist2"].max()


def test_sphere_shell_mass_ties_at_the_centre(mv):
    p = full(32) - 16
    r2 = (p * p).sum(1)
    _, want = check(mv, (p + 16)[(r2 <= 13 * 13) & (r2 > 12 * 12)], 32)
    assert want["dist2"].max() >= 12 * 12 and want["nRegions"] == 1


def test_two_cavities_behind_a_one_voxel_wall_and_nested_shells(mv):
    _, want = check(mv, np.concatenate([shell((1, 1, 1), (8, 8, 8)), shell((7, 1, 1), (14, 8, 8))]), 16)
    assert want["nRegions"] == 2
    _, want = check(mv, np.concatenate([shell(2, 14), shell(5, 11)]), 16)
    assert want["nRegions"] == 2 and np.bincount(want["region"]).tolist() == [10 ** 3 - 6 ** 3, 4 ** 3]


def test_far_corner_of_the_largest_grid(mv):
    res = 1 << 21
    xyz = np.concatenate([shell(res - 7, res - 1), [(res - 4, res - 5, res - 4)]])
    svo = build(mv, xyz, res)
    x0, a0 = svo.read_voxels()
    cells = full(4) + res - 6
    cells = cells[~(cells == (res - 4, res - 5, res - 4)).all(1)]
    cells = cells[np.argsort(S.morton(cells), kind="stable")]
    d2, near = N.nearest_of(cells, x0)  # (the dense model does not reach this far; the cells of this shape are known)
    got = svo.enclosed_nearest()
    assert np.array_equal(got["xyz"], cells) and got["nRegions"] == 1 and (got["region"] == 0).all()
    assert np.array_equal(got["dist2"], d2) and np.array_equal(got["nearest"], near) and np.array_equal(got["attribs"], N._alpha255(a0[near]))
    assert svo.fill_enclosed_nearest() == 63 and svo.enclosed_nearest_device() == (0, 0)


def test_serpentine_corridor(mv):
    solid, path = serpentine()
    _, want = check(mv, np.argwhere(solid), 32)
    assert len(want["xyz"]) == len(path) and (want["dist2"] == 1).all()


def test_grids_without_an_enclosed_cell(mv):
    for xyz, res in ((full(4), 4), ([(1, 0, 1)], 2), (open_cage(), 8)):
        svo = build(mv, xyz, res)
        xyz_d, hx = filled(mv, (4, 3), np.uint32)
        assert svo.enclosed_nearest_device(4, xyz_d) == (0, 0) and np.array_equal(xyz_d.to_host(), hx)
        got = svo.enclosed_nearest()
        assert all(len(got[k]) == 0 for k in KEYS) and got["nRegions"] == 0
        before = octree(svo)
        assert svo.fill_enclosed_nearest() == 0 and same(octree(svo), before)


# ---- flavours, edits, uploads, steps in flight -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_every_flavour(mv, flags):
    xyz = debris_cavity(16, 8, 6, 2)
    svo, want = check(mv, xyz, 16, flags)
    assert flags != 3 or svo.info().flavour == 2
    flavour = svo.info().flavour
    assert_fill(mv, xyz, 16, flags)
    assert svo.fill_enclosed_nearest() == len(want["xyz"]) and svo.info().flavour == flavour


def test_after_an_edit_after_a_fill_and_a_rebuilt_upload(mv):
    svo = build(mv, debris_cavity(16, 8, 6, 2), 16)
    svo.edit_voxels(np.array([(7, 7, 7), (1, 1, 1)], np.uint32), colours(2, 8))
    svo.edit_voxels(np.array([(3, 3, 3)], np.uint32), None, np.zeros(1, np.uint8))  # a corner of the shell goes: still closed for 6-connectivity
    want = assert_listing(svo, 16)
    assert len(want["xyz"]) > 400
    nodes, attrs, _ = svo.download()
    i = svo.info()
    up = mv.IntersectorOctreeGPU()
    up.upload(nodes, attrs, LOWER, DPS, 16, i.hasEmission, embeddedMask=bool(i.embeddedMask))
    for call in (up.enclosed_nearest_device, up.fill_enclosed_nearest):
        with pytest.raises(mv.MvrtError, match="keeps no Morton codes"):
            call()
    up.rebuild()
    assert_listing(up, 16, want)
    assert svo.fill_enclosed_nearest() == len(want["xyz"])
    assert svo.enclosed_nearest_device() == (0, 0) and svo.fill_enclosed_nearest() == 0  # after a first fill: nothing is left


def test_refusals_without_gpu_work(mv):
    empty = mv.IntersectorOctreeGPU()
    allocs = mv.allocation_state()[2]
    for call in (empty.enclosed_nearest_device, empty.fill_enclosed_nearest):
        with pytest.raises(mv.MvrtError, match="no octree"):
            call()
    assert mv.allocation_state()[2] == allocs


def bunny(mv, conservative=False):
    v = bunny_tris().reshape(-1, 3)
    lo = v.min(0)
    dps = np.float32((v.max(0) - lo).max() / np.float32(64))
    base = mv.IntersectorOctreeGPU()
    base.build(v, None, None, None, lo, dps, 64, flags=mv.IntersectorOctreeGPU.BUILD_CONSERVATIVE if conservative else 0)
    x0, _ = base.read_voxels()
    svo = mv.IntersectorOctreeGPU()
    svo.build_voxels(x0, colours(len(x0), 12), origin=lo, dps=dps, gridRes=64)
    return svo


@pytest.fixture(scope="module")
def bunny_case(mv):
    svo = bunny(mv)
    x0, a0 = svo.read_voxels()
    return svo, N.enclosed_nearest(x0, a0, 64)


def test_bunny_at_64(mv, bunny_case):
    svo, want = bunny_case
    assert (svo.info().numberOfVoxels, len(want["xyz"]), want["nRegions"]) == (8516, 48162, 3)
    assert_listing(svo, 64, want)
    print(mv.enclosed_nearest_stats())


def test_bunny_at_64_conservative(mv):
    svo = bunny(mv, True)
    want = assert_listing(svo, 64)
    assert (svo.info().numberOfVoxels, len(want["xyz"])) == (13774, 45658)


def assert_agrees_with_the_band(svo, got):
    band = svo.distance_cells(1024)
    index = {int(c): i for i, c in enumerate(S.morton(band["xyz"]))}
    codes = S.morton(got["xyz"])
    within = got["dist2"] <= 1024
    at = np.array([index[int(c)] for c in codes[within]], np.int64)
    assert within.any() and all(int(c) not in index or w for c, w in zip(codes, within))
    for k in ("dist2", "nearest", "attribs"):
        assert np.array_equal(band[k][at], got[k][within]), k


def test_agreement_with_the_band_engine(mv, bunny_case):
    svo = build(mv, debris_cavity(), 32)
    assert_agrees_with_the_band(svo, svo.enclosed_nearest())
    assert_agrees_with_the_band(bunny_case[0], bunny_case[0].enclosed_nearest())


def test_cells_and_regions_equal_enclosed_cells(mv, bunny_case):
    for svo in (bunny_case[0], build(mv, np.concatenate([shell(2, 14), shell(5, 11)]), 16)):
        a, b = svo.enclosed_cells(), svo.enclosed_nearest()
        assert np.array_equal(a["xyz"], b["xyz"]) and np.array_equal(a["region"], b["region"]) and a["nRegions"] == b["nRegions"]


def test_through_the_path_tracers_intersector_with_steps_in_flight(mv):
    """The same two steps around the fill and around the edit it stands for: the step issued before finishes first on the old octree, the frame buffer is not
    cleared, and the second step accumulates on it."""
    v = bunny_tris().reshape(-1, 3)
    lo = v.min(0)
    res, w, h = 32, 64, 36
    dps = np.float32((v.max(0) - lo).max() / np.float32(res))
    rgba, hw, hh = mv.read_rgbe_file(os.path.join(GOLDEN, "monks_forest_s.hdr"))
    cam = probe_camera(lo, dps, res, focus=9.0, lens_r=0.05)
    frames = []
    for use_call in (True, False):
        pt = mv.PathTracer()
        pt.setup(None)
        pt.resizeFrameBufferIfNeeded(None, w, h)
        pt.loadHDRIPixels(None, rgba, hw, hh, rgba, hw, hh)
        svo = pt.m_intersectorOctreeGPU
        svo.build(v, None, None, None, lo, dps, res)
        x0, a0 = svo.read_voxels()
        want = N.enclosed_nearest(x0, a0, res)
        assert len(want["xyz"]) > 0
        pt.step(None, cam)
        if use_call:
            assert svo.fill_enclosed_nearest() == len(want["xyz"])
        else:
            svo.edit_voxels(want["xyz"], want["attribs"])
        assert svo.info().numberOfVoxels == len(x0) + len(want["xyz"])
        pt.step(None, cam)
        assert pt.getSteps() == 2
        frames.append(pt.read_framebuffer()[: w * h].copy())
        pt.cleanUp()
    assert np.array_equal(frames[0].view(np.uint32), frames[1].view(np.uint32))


# ---- the contract ------------------------------------------------------------------------------------------------------------------------------------------------
def test_null_outputs_and_capacity(mv):
    svo = build(mv, debris_cavity(16, 8, 6, 2), 16)
    before, info, held = octree(svo), bytes(svo.info()), mv.allocation_state()[:2]
    want = assert_listing(svo, 16)
    n = len(want["xyz"])
    shapes = {"xyz": ((n, 3), np.uint32), "region": (n, np.uint32), "dist2": (n, np.uint32), "nearest": (n, np.uint32), "attribs": ((n, 8), np.uint8)}
    for k in KEYS:  # each output alone, the others NULL
        out = mv.DeviceArray(*shapes[k])
        assert svo.enclosed_nearest_device(n, **{k: out}) == (n, want["nRegions"]) and np.array_equal(out.to_host(), want[k]), k
    for k in KEYS:  # each output NULL in turn
        outs = {j: mv.DeviceArray(*shapes[j]) for j in KEYS if j != k}
        assert svo.enclosed_nearest_device(n, **outs) == (n, want["nRegions"])
        assert all(np.array_equal(outs[j].to_host(), want[j]) for j in outs), k
    lib = mv.lib()
    assert lib.mvrt_svo_enclosed_nearest(svo._h, 0, None, None, None, None, None, None, None, None) == 0  # even the counts may be NULL
    # one short: the counts are still returned and nothing is written
    arrays = {k: filled(mv, *shapes[k]) for k in KEYS}
    nc, nr = C.c_uint64(0), C.c_uint64(0)
    assert lib.mvrt_svo_enclosed_nearest(svo._h, n - 1, *[arrays[k][0].ptr for k in KEYS], C.byref(nc), C.byref(nr), None) != 0
    assert (nc.value, nr.value) == (n, want["nRegions"]) and b"capacity %d" % (n - 1) in lib.mvrt_last_error()
    assert all(np.array_equal(arrays[k][0].to_host(), arrays[k][1]) for k in KEYS)
    assert bytes(svo.info()) == info and same(octree(svo), before) and mv.allocation_state()[:2] == held  # never modified, the scratch is gone


# ---- the fill ----------------------------------------------------------------------------------------------------------------------------------------------------
def assert_fill(mv, xyz, res, flags=0, emission=True):
    a, b = build(mv, xyz, res, flags, emission=emission), build(mv, xyz, res, flags, emission=emission)
    x0, a0 = a.read_voxels()
    want = N.enclosed_nearest(x0, a0, res)
    assert a.fill_enclosed_nearest() == len(want["xyz"]) > 0
    assert same(a.read_voxels(), N.filled(x0, a0, res))
    b.edit_voxels(want["xyz"], want["attribs"])
    assert_same_octree(a, b)
    return a, want


def test_fill_equals_an_edit_with_the_models_cells(mv):
    a, want = assert_fill(mv, debris_cavity(), 32)
    assert a.info().hasEmission == 1 and want["attribs"][:, 4:7].any()
    a, want = assert_fill(mv, debris_cavity(), 32, emission=False)
    assert a.info().hasEmission == 0 and not want["attribs"][:, 4:7].any()


def test_fill_with_zero_cells_leaves_the_handle_untouched(mv):
    svo = build(mv, open_cage(), 8)
    before, info, view = octree(svo), bytes(svo.info()), bytes(svo.device_view())
    assert svo.fill_enclosed_nearest() == 0
    assert bytes(svo.info()) == info and same(octree(svo), before) and bytes(svo.device_view()) == view
