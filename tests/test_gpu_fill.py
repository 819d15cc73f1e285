"""Enclosed empty cells and the fill on the GPU (mvrt_svo_enclosed_cells / mvrt_svo_fill_enclosed) against the numpy model of tests/fill_expected.py: xyz,
region, nCells and nRegions bit for bit, on the smallest inputs that can break each mechanism -- grids without a gap, a one-cell cage, diagonal contact, a shell
on the grid border, one long gap (the neighbour walk), several hundred chained gaps (the depth of the union-find and its propagation across launch blocks),
nesting and numbering, random fills across every 256-item seam, lists of 255 to 612 voxels with cells on both sides of a seam and a group without any, the 21-bit edge, every flavour, edits, a rebuilt upload, the bunny -- and the contract of the two
calls.  The listing limit (nCells >= 2^32) and the fill limit (numberOfVoxels + nCells >= 2^32 - 1) are host comparisons (csrc/kernels_fill.hip, csrc/api.hip)
covered by reading: reaching them takes 2^32 cells."""
import ctypes as C
import os

import numpy as np
import pytest

import fill_expected as F
import surface_expected as S
from common import GOLDEN, bunny_tris, probe_camera
from fixtures import mv  # noqa: F401 (fixtures)
from voxel_sets import CAGE, DPS, LOWER, assert_same_octree, filled, filler, full, serpentine, shell, tube

pytestmark = pytest.mark.gpu


def build(mv, xyz, res, flags=0, attribs=None):
    svo = mv.IntersectorOctreeGPU()
    svo.build_voxels(np.ascontiguousarray(xyz, np.uint32), attribs, origin=LOWER, dps=DPS, gridRes=res, flags=flags)
    return svo


def assert_cells(svo, want):
    got = svo.enclosed_cells()
    n = len(want["xyz"])
    print("cells", len(got["xyz"]), "regions", got["nRegions"], "model", n, want["nRegions"])
    assert svo.enclosed_cells_device() == (n, want["nRegions"])  # the sizing call
    assert got["xyz"].shape == (n, 3) and got["xyz"].dtype == np.uint32 and np.array_equal(got["xyz"], want["xyz"])
    assert got["region"].dtype == np.uint32 and np.array_equal(got["region"], want["region"]) and got["nRegions"] == want["nRegions"]


def check(mv, xyz, res, flags=0):
    want = F.enclosed(xyz, res)
    svo = build(mv, xyz, res, flags)
    assert_cells(svo, want)
    return svo, want


# ---- tiny grids, the cage, diagonal contact, the border --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [2, 4])
def test_grids_without_a_gap(mv, res):
    _, want = check(mv, full(res), res)  # a full grid: success with both counts 0
    assert len(want["xyz"]) == 0 and want["nRegions"] == 0
    check(mv, [(1, 0, 1)], res)
    check(mv, [(0, 0, 0), (res - 1, 0, 0), (0, res - 1, res - 1)], res)


def test_cage(mv):
    _, want = check(mv, CAGE, 4)
    assert want["xyz"].tolist() == [[1, 1, 1]] and want["nRegions"] == 1
    for gone in range(6):
        _, w = check(mv, CAGE[:gone] + CAGE[gone + 1:], 4)
        assert len(w["xyz"]) == 0


def test_diagonal_contact_gives_two_regions(mv):
    solid = np.ones((4, 4, 3), bool)
    solid[1, 1, 1] = solid[2, 2, 1] = False
    _, want = check(mv, np.argwhere(solid), 8)
    assert want["region"].tolist() == [0, 1]


def test_shell_on_the_grid_border(mv):
    _, want = check(mv, shell(0, 8), 8)
    assert len(want["xyz"]) == 216 and want["nRegions"] == 1


# ---- one long gap: the neighbour walk; many chained gaps: the union-find -----------------------------------------------------------------------------------------
def test_one_long_gap(mv):
    t = tube()
    _, want = check(mv, t, 512)
    assert len(want["xyz"]) == 298 and want["nRegions"] == 1
    cap = (t == (399, 11, 21)).all(1)
    assert cap.sum() == 1
    _, w = check(mv, t[~cap], 512)
    assert len(w["xyz"]) == 0


def test_many_chained_gaps(mv):
    solid, path = serpentine()
    lin = np.sort((path[:, 2] * 32 + path[:, 1]) * 32 + path[:, 0])
    n_gaps = 1 + int((np.diff(lin) != 1).sum())
    assert n_gaps > 400  # several hundred gaps in one chain, over more than one launch block of gaps
    _, want = check(mv, np.argwhere(solid), 32)
    assert len(want["xyz"]) == len(path) and want["nRegions"] == 1
    # the voxel behind the corridor's far end, on the grid border: without it everything is exterior
    end = path[-1].copy()
    assert end[0] in (1, 30)
    end[0] = 0 if end[0] == 1 else 31
    opened = solid.copy()
    opened[tuple(end)] = False
    _, w = check(mv, np.argwhere(opened), 32)
    assert len(w["xyz"]) == 0 and w["nRegions"] == 0


# ---- nesting and numbering ---------------------------------------------------------------------------------------------------------------------------------------------
def test_nested_shells(mv):
    _, want = check(mv, np.concatenate([shell(2, 14), shell(5, 11)]), 16)
    assert want["nRegions"] == 2 and np.bincount(want["region"]).tolist() == [10 ** 3 - 6 ** 3, 4 ** 3]


def test_regions_are_numbered_by_first_morton_appearance(mv):
    a, b = shell((9, 1, 1), (15, 7, 7)), shell((1, 1, 2), (7, 7, 8))  # a comes first by (z, y, x), b by Morton code
    _, want = check(mv, np.concatenate([a, b]), 16)
    assert want["nRegions"] == 2 and want["xyz"][0, 0] < 7 and want["region"][0] == 0
    first_of_a = np.argmax(want["xyz"][:, 0] > 8)
    assert want["region"][first_of_a] == 1 and (want["region"][:first_of_a] == 0).all()


# ---- random fills ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("density", [0.5, 0.7, 0.85])
@pytest.mark.parametrize("res", [16, 32])
def test_random_fill(mv, res, density, seed):
    rng = np.random.default_rng(1000 * res + 10 * int(density * 10) + seed)
    xyz = np.argwhere(rng.random((res, res, res)) < density)
    border = [(0, 1, 2), (res - 1, 2, 1), (1, 0, 2), (2, res - 1, 1), (2, 1, 0), (1, 2, res - 1)]  # all six grid borders
    check(mv, np.concatenate([xyz, border]), res)


def test_random_fills_have_many_small_regions():
    """(the model alone) the random sets above are worth their time: dozens of regions at 32^3"""
    rng = np.random.default_rng(1000 * 32 + 10 * 7 + 0)
    assert F.enclosed(np.argwhere(rng.random((32, 32, 32)) < 0.7), 32)["nRegions"] >= 24


# ---- the seams of the emit kernel's groups -----------------------------------------------------------------------------------------------------------------------
def emitted_per_gap(xyz, res, want):
    """per voxel i of the list sorted by (z, y, x) -- the order the emit kernel's groups of 256 are cut from -- the enclosed cells of the gap between voxels i
    and i + 1 (0: no gap, or an exterior one), from the model's cells"""
    p = np.asarray(xyz, np.int64)
    lin = np.sort((p[:, 2] * res + p[:, 1]) * res + p[:, 0])
    length = np.where(lin[1:] // res == lin[:-1] // res, lin[1:] - lin[:-1] - 1, 0)
    w = want["xyz"].astype(np.int64)
    inside = np.isin(lin[:-1] + 1, (w[:, 2] * res + w[:, 1]) * res + w[:, 0])  # (a gap is enclosed or exterior as a whole: its first cell decides)
    out = np.append(np.where(inside, length, 0), 0)
    assert out.sum() == len(w)
    return out


def seam_scene(n):
    """n voxels at gridRes 32, in (z, y, x) order: a cage, a layer of filler, [two cages that share a voxel, a layer of filler,] a cage"""
    cage = np.array(CAGE)
    if n == 513:  # the two gaps of the double cage are items 255 and 256: the last of the first group and the first of the second
        double = np.unique(np.concatenate([cage + (0, 0, 6), cage + (2, 0, 6)]), axis=0)
        assert len(double) == 11
        middle = [filler(245, 4), double, filler(n - 6 - 245 - 11 - 6, 10)]
    else:
        middle = [filler(n - 12, 4)]
    xyz = np.concatenate([cage] + middle + [cage + (5, 5, 12)])
    assert len(xyz) == n == len(np.unique(xyz, axis=0))
    return xyz


@pytest.mark.parametrize("n", [255, 256, 257, 513, 612])
def test_voxel_counts_at_the_group_seams(mv, n):
    xyz = seam_scene(n)
    svo, want = check(mv, xyz, 32)
    cells = emitted_per_gap(xyz, 32, want)
    groups = [int(cells[g:g + 256].sum()) for g in range(0, n, 256)]
    print(n, "cells per group", groups)
    assert cells[2] == 1 and cells[n - 4] == 1  # the first cage's gap and the last one's, four items before the end
    if n == 513:
        assert cells[255] == 1 and cells[256] == 1 and groups == [2, 2, 0]
    elif n == 612:  # a whole group without a cell between two that have one
        assert groups == [1, 0, 1]
    else:
        assert groups == [2] + [0] * (len(groups) - 1)
    assert svo.fill_enclosed() == len(want["xyz"])  # the emit's other output: the cells as they come
    assert np.array_equal(svo.read_voxels()[0], F.filled_set(xyz, 32))


def test_a_gap_longer_than_a_group(mv):
    """the tube's one gap has more cells than a group has threads and than a group has items: every thread takes a second cell of the same item"""
    t = tube()
    svo, want = check(mv, t, 512)
    cells = emitted_per_gap(t, 512, want)
    assert cells.max() == 298 > 256 and (cells > 0).sum() == 1
    assert svo.fill_enclosed() == 298 and np.array_equal(svo.read_voxels()[0], F.filled_set(t, 512))


# ---- the 21-bit edge -------------------------------------------------------------------------------------------------------------------------------------------------
def test_far_corner_of_the_largest_grid(mv):
    res = 1 << 21
    svo, want = check(mv, shell(res - 5, res), res)
    assert svo.info().levels == 21 and len(want["xyz"]) == 27 and want["xyz"].max() == res - 2


# ---- flavours, edits, uploads, triangle builds -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed():
    rng = np.random.default_rng(77)
    xyz = np.concatenate([np.argwhere(rng.random((32, 32, 32)) < 0.7), shell(3, 12)])
    return xyz, F.enclosed(xyz, 32)


@pytest.mark.parametrize("flags", [1, 2, 3])
def test_every_flavour_gives_the_same_bytes(mv, mixed, flags):
    xyz, want = mixed
    assert want["nRegions"] > 10
    svo = build(mv, xyz, 32, flags)
    assert flags != 3 or svo.info().flavour == 2  # the tree flavour
    assert_cells(svo, want)
    assert_cells(build(mv, xyz, 32, 0), want)


def test_after_edits_seal_and_unseal_a_cavity(mv):
    at = np.array(CAGE) + 3
    svo, want = check(mv, at[:5], 8)
    assert len(want["xyz"]) == 0
    svo.edit_voxels(at[5:].astype(np.uint32))
    sealed = F.enclosed(at, 8)
    assert sealed["xyz"].tolist() == [[4, 4, 4]]
    assert_cells(svo, sealed)
    svo.edit_voxels(at[2:3].astype(np.uint32), None, np.zeros(1, np.uint8))
    assert_cells(svo, want)


def test_after_rebuild_of_an_upload(mv, mixed):
    xyz, want = mixed
    svo = build(mv, xyz, 32)
    nodes, attrs, _ = svo.download()
    i = svo.info()
    up = mv.IntersectorOctreeGPU()
    up.upload(nodes, attrs, LOWER, DPS, 32, i.hasEmission, embeddedMask=bool(i.embeddedMask))
    with pytest.raises(mv.MvrtError, match="keeps no Morton codes"):
        up.enclosed_cells_device()
    up.rebuild()
    assert_cells(up, want)


@pytest.mark.parametrize("conservative", [False, True])
def test_bunny_from_triangles(mv, conservative):
    tris = bunny_tris()
    v = tris.reshape(-1, 3)
    lo = v.min(0)
    dps = np.float32((v.max(0) - lo).max() / np.float32(64))
    svo = mv.IntersectorOctreeGPU()
    svo.build(v, None, None, None, lo, dps, 64, flags=mv.IntersectorOctreeGPU.BUILD_CONSERVATIVE if conservative else 0)
    xyz, _ = svo.read_voxels()
    want = F.enclosed(xyz, 64)
    assert_cells(svo, want)
    assert (len(xyz), len(want["xyz"])) == ((13774, 45658) if conservative else (8516, 48162))  # the oracle's voxel sets (tests/test_fill_cpu.py)


@pytest.mark.parametrize("res,voxels,cells", [(128, 33487, 401846), (256, 133016, 3281611)])
def test_bunny_counts_at_larger_grids_repeat(mv, res, voxels, cells):
    """The counts a dense host flood fill of the oracle's six-separating voxel set gives at these grids (the model here would take minutes): unions over tens of
    thousands of gaps in one deep set, where a lost union or a flattened entry that is no root shows as a count that is too high or changes from call to call.
    Every listed cell is empty, distinct and in Morton order, and the large cavity is one region."""
    tris = bunny_tris()
    v = tris.reshape(-1, 3)
    lo = v.min(0)
    svo = mv.IntersectorOctreeGPU()
    svo.build(v, None, None, None, lo, np.float32((v.max(0) - lo).max() / np.float32(res)), res)
    assert svo.info().numberOfVoxels == voxels
    counts = {svo.enclosed_cells_device() for _ in range(8)}
    print(res, counts)
    assert len(counts) == 1 and counts.pop()[0] == cells
    got = svo.enclosed_cells()
    codes = S.morton(got["xyz"])
    assert len(codes) == cells and (np.diff(codes.astype(np.int64)) > 0).all() and not np.isin(codes, S.morton(svo.read_voxels()[0])).any()
    assert got["region"][0] == 0 and np.bincount(got["region"]).max() > 0.99 * cells and got["region"].max() + 1 == got["nRegions"]
    seen = np.maximum.accumulate(got["region"])
    assert (got["region"][1:] <= seen[:-1] + 1).all()  # a new id is always the previous maximum + 1


# ---- the contract of the listing -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(mv, mixed):
    xyz, want = mixed
    return build(mv, xyz, 32), want


def test_null_outputs(mv, small):
    svo, want = small
    n, nr = len(want["xyz"]), want["nRegions"]
    assert svo.enclosed_cells_device() == (n, nr)  # capacity 0, all NULL
    xyz, region = mv.DeviceArray((n, 3), np.uint32), mv.DeviceArray(n, np.uint32)
    assert svo.enclosed_cells_device(n, xyz, None) == (n, nr) and np.array_equal(xyz.to_host(), want["xyz"])
    assert svo.enclosed_cells_device(n, None, region) == (n, nr) and np.array_equal(region.to_host(), want["region"])
    lib = mv.lib()
    nc = C.c_uint64(0)
    assert lib.mvrt_svo_enclosed_cells(svo._h, 0, None, None, None, None, None) == 0  # even the counts may be NULL
    assert lib.mvrt_svo_enclosed_cells(svo._h, 0, None, None, C.byref(nc), None, None) == 0 and nc.value == n
    nc.value = 0
    assert lib.mvrt_svo_enclosed_cells(svo._h, 0, None, None, None, C.byref(nc), None) == 0 and nc.value == nr
    # a larger capacity than the count is fine and writes the count's worth
    big, host = filled(mv, (n + 5, 3), np.uint32)
    assert svo.enclosed_cells_device(n + 5, big, None) == (n, nr)
    assert np.array_equal(big.to_host()[:n], want["xyz"]) and np.array_equal(big.to_host()[n:], host[n:])


def test_capacity_one_short(mv, small):
    svo, want = small
    n, nr = len(want["xyz"]), want["nRegions"]
    (xyz, xyz_host), (region, region_host) = filled(mv, (n, 3), np.uint32), filled(mv, n, np.uint32)
    lib = mv.lib()
    nc, nreg = C.c_uint64(0), C.c_uint64(0)
    assert lib.mvrt_svo_enclosed_cells(svo._h, n - 1, xyz.ptr, region.ptr, C.byref(nc), C.byref(nreg), None) != 0
    assert (nc.value, nreg.value) == (n, nr) and b"capacity %d" % (n - 1) in lib.mvrt_last_error() and b"%d enclosed cells" % n in lib.mvrt_last_error()
    assert np.array_equal(xyz.to_host(), xyz_host) and np.array_equal(region.to_host(), region_host)  # nothing was written
    with pytest.raises(mv.MvrtError, match="capacity"):
        svo.enclosed_cells_device(n - 1, None, region)
    assert np.array_equal(region.to_host(), region_host)


def test_refusals_without_gpu_work(mv, small):
    svo, _ = small
    empty = mv.IntersectorOctreeGPU()
    nodes, attrs, _ = svo.download()
    i = svo.info()
    up = mv.IntersectorOctreeGPU()
    up.upload(nodes, attrs, LOWER, DPS, 32, i.hasEmission, embeddedMask=bool(i.embeddedMask))
    before = mv.allocation_state()[2]
    for h, text in ((empty, "no octree"), (up, "keeps no Morton codes")):
        for call in (h.enclosed_cells_device, h.fill_enclosed):
            with pytest.raises(mv.MvrtError, match=text):
                call()
    assert mv.allocation_state()[2] == before


def test_the_handle_is_not_modified(mv, small):
    svo, want = small
    before = svo.download(want_morton=True)
    info = bytes(svo.info())
    held = mv.allocation_state()[:2]
    assert_cells(svo, want)
    assert bytes(svo.info()) == info and all(np.array_equal(a, b) for a, b in zip(svo.download(want_morton=True), before))
    assert mv.allocation_state()[:2] == held  # the scratch is gone


# ---- the fill ----------------------------------------------------------------------------------------------------------------------------------------------------------
RED_GLOW = np.array([200, 10, 20, 7, 90, 0, 0, 9], np.uint8)  # emissive; both alpha bytes are stored as 255


@pytest.mark.parametrize("flags", [0, 3])
@pytest.mark.parametrize("attrib", [None, RED_GLOW])
def test_fill_equals_an_edit_with_the_models_cells(mv, mixed, attrib, flags):
    xyz, want = mixed
    rng = np.random.default_rng(4)
    attrs = rng.integers(0, 256, size=(len(xyz), 8), dtype=np.uint8)
    attrs[:, 4:7] = 0  # no emission before the fill
    a, b = build(mv, xyz, 32, flags, attrs), build(mv, xyz, 32, flags, attrs)
    a.set_emission_scale(3.25)
    b.set_emission_scale(3.25)
    n = len(want["xyz"])
    old_xyz, old_attrs = a.read_voxels()
    assert a.info().hasEmission == 0
    assert a.fill_enclosed(attrib) == n
    b.edit_voxels(want["xyz"], None if attrib is None else np.tile(attrib, (n, 1)))
    assert_same_octree(a, b)
    assert a.info().hasEmission == (0 if attrib is None else 1) and a.info().numberOfVoxels == len(old_xyz) + n
    new_xyz, new_attrs = a.read_voxels()
    was = np.isin(S.morton(new_xyz), S.morton(old_xyz))
    assert np.array_equal(new_attrs[was], old_attrs) and was.sum() == len(old_xyz)  # existing voxels keep their attributes
    fill = np.array([255, 255, 255, 255, 0, 0, 0, 255], np.uint8) if attrib is None else np.array([200, 10, 20, 255, 90, 0, 0, 255], np.uint8)
    assert (new_attrs[~was] == fill).all() and np.array_equal(new_xyz[~was], want["xyz"])
    # nothing is enclosed any more: a second fill is a no-op
    before = a.download(want_morton=True)
    view = bytes(a.device_view()) if flags == 0 else None
    assert a.fill_enclosed(attrib) == 0 and a.enclosed_cells_device() == (0, 0)
    assert all(np.array_equal(x, y) for x, y in zip(a.download(want_morton=True), before))
    assert view is None or bytes(a.device_view()) == view
    # the surface of the filled set
    surf = S.surface(F.filled_set(xyz, 32), 32, LOWER, DPS)
    masks, nf = a.surface_masks()
    assert np.array_equal(masks, surf["masks"]) and nf == surf["nFaces"]


def test_a_set_without_cavities_is_untouched_and_its_view_stays_valid(mv):
    rng = np.random.default_rng(9)
    xyz = np.argwhere(rng.random((32, 32, 32)) < 0.05)
    assert len(F.enclosed(xyz, 32)["xyz"]) == 0
    svo = build(mv, xyz, 32)
    ro = np.tile((LOWER + DPS * 32 * np.array([1.6, 1.3, 1.4], np.float32)).astype(np.float32), (2000, 1))  # outside the grid, aimed at points inside it
    rd = (LOWER + DPS * 32 * rng.random((2000, 3)).astype(np.float32) - ro).astype(np.float32)
    hits = svo.intersect_range(ro, rd, np.float32(3.0e38))
    assert (hits["nMajor"] >= 0).sum() > 200
    view, octree, allocs = bytes(svo.device_view()), svo.download(want_morton=True), mv.allocation_state()[:2]
    assert svo.fill_enclosed() == 0
    assert bytes(svo.device_view()) == view and mv.allocation_state()[:2] == allocs  # the same arrays at the same addresses: no rebuild
    assert all(np.array_equal(x, y) for x, y in zip(svo.download(want_morton=True), octree))
    again = svo.intersect_range(ro, rd, np.float32(3.0e38))  # (this trace runs on the device view)
    assert all(np.array_equal(hits[k], again[k]) for k in hits)


def test_fill_through_the_path_tracers_intersector_between_steps(mv):
    """The same two steps around a fill and around the edit it stands for: the step issued before the fill finishes first on the old octree, the frame buffer is
    not cleared, and the second step accumulates on it.  (That an edit between steps renders like the oracle is test_gpu_voxel_edit.py's.)"""
    tris = bunny_tris()
    v = tris.reshape(-1, 3)
    lo = v.min(0)
    res, w, h = 64, 64, 36
    dps = np.float32((v.max(0) - lo).max() / np.float32(res))
    rgba, hw, hh = mv.read_rgbe_file(os.path.join(GOLDEN, "monks_forest_s.hdr"))
    cam = probe_camera(lo, dps, res, focus=9.0, lens_r=0.05)
    frames = []
    for use_fill in (True, False):
        pt = mv.PathTracer()
        pt.setup(None)
        pt.resizeFrameBufferIfNeeded(None, w, h)
        pt.loadHDRIPixels(None, rgba, hw, hh, rgba, hw, hh)
        svo = pt.m_intersectorOctreeGPU
        svo.build(v, None, None, None, lo, dps, res)
        xyz, _ = svo.read_voxels()
        pt.step(None, cam)
        if use_fill:
            assert svo.fill_enclosed(RED_GLOW) == 48162
        else:
            cells = F.enclosed(xyz, res)["xyz"]
            svo.edit_voxels(cells, np.tile(RED_GLOW, (len(cells), 1)))
        assert svo.info().numberOfVoxels == len(xyz) + 48162 and svo.info().hasEmission == 1
        pt.step(None, cam)
        assert pt.getSteps() == 2
        frames.append(pt.read_framebuffer()[: w * h].copy())
        pt.cleanUp()
    assert np.array_equal(frames[0], frames[1]) and frames[0].max() > 0
