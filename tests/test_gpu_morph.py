"""Dilation, erosion, closing and opening on the GPU (mvrt_svo_dilation_cells / _erosion_voxels / _dilate / _erode / _close / _open) against the numpy model of
tests/morph_expected.py, bit for bit: the listings array by array, the in-place calls through read_voxels, the identity with the edit through download() of a
second handle that was given the listing via edit_voxels.  On the smallest inputs that can break each mechanism -- a corner voxel and the full grid at gridRes 2,
a centre voxel, two voxels across the top octant seam with a cell both reach, the floor of a 26-colour mean, rows of 255 to 513 voxels with every second cell
empty, a solid block whose sorted list holds a 256-aligned stretch without records, the borders and corners of the 2^21 grid, several steps in one call, every
flavour, edits, fills, a rebuilt upload, steps in flight, the holed shell, the bunny -- and the contract of the six calls.  The count limits (a step whose pairs
or whose voxels would reach 2^32 - 1) are host comparisons (csrc/kernels_morph.hip) covered by reading: reaching them takes 2^32 entries."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import morph_expected as M
import surface_expected as S
from common import GOLDEN, bunny_tris, probe_camera
from fixtures import mv  # noqa: F401 (fixtures)
from voxel_sets import DPS, LOWER, assert_same_octree, build, colours, filled, full, holed_shell, octree, same, specks_and_block

pytestmark = pytest.mark.gpu

ELEMENTS = (M.FACES, M.CUBE)
OPS = ("dilate", "erode", "close", "open")


def assert_listings(svo, res, sparse=False):
    x0, a0 = svo.read_voxels()
    for e in ELEMENTS:
        want, got = M.dilation_cells(x0, a0, res, e, sparse), svo.dilation_cells(e)
        n = len(want["xyz"])
        print("element", e, "dilation cells", len(got["xyz"]), "model", n)
        assert svo.dilation_cells_device(e) == n  # the sizing call
        assert got["xyz"].shape == (n, 3) and got["xyz"].dtype == np.uint32 and np.array_equal(got["xyz"], want["xyz"])
        assert got["attribs"].shape == (n, 8) and np.array_equal(got["attribs"], want["attribs"])
        assert got["count"].dtype == np.uint32 and np.array_equal(got["count"], want["count"])
        gone, peeled = M.erosion_voxels(x0, res, e, sparse), svo.erosion_voxels(e)
        print("element", e, "erosion voxels", len(peeled), "model", len(gone))
        assert svo.erosion_voxels_device(e) == len(gone) and peeled.dtype == np.uint32 and np.array_equal(peeled, gone)


def assert_op(mv, xyz, res, op, e, steps, flags=0, attribs=None, sparse=False):
    """one in-place call on a fresh build against the model; a call that would leave no voxel is refused with the handle byte-identical"""
    svo = build(mv, xyz, res, flags, attribs)
    x0, a0 = svo.read_voxels()
    wx, wa = M.morph(op, x0, a0, res, e, steps, sparse)
    before, info = octree(svo), bytes(svo.info())
    if len(wx) == 0:
        with pytest.raises(mv.MvrtError, match="would leave no voxel"):
            getattr(svo, op)(e, steps)
        assert bytes(svo.info()) == info and same(octree(svo), before)
        return svo
    n = getattr(svo, op)(e, steps)
    gx, ga = svo.read_voxels()
    print(op, "element", e, "steps", steps, "voxels", len(x0), "->", len(gx), "model", len(wx), "returned", n)
    assert n == abs(len(wx) - len(x0)) and svo.info().numberOfVoxels == len(wx)
    assert np.array_equal(gx, wx) and np.array_equal(ga, wa)
    assert svo.info().hasEmission == int(wa[:, 4:7].any())
    if n == 0:
        assert bytes(svo.info()) == info and same(octree(svo), before)
    return svo


def assert_all(mv, xyz, res, flags=0, attribs=None, sparse=False, steps=(1,)):
    assert_listings(build(mv, xyz, res, flags, attribs), res, sparse)
    for op, e, k in itertools.product(OPS, ELEMENTS, steps):
        assert_op(mv, xyz, res, op, e, k, flags, attribs, sparse)


# ---- the smallest grids ----------------------------------------------------------------------------------------------------------------------------------------
def test_corner_voxel_at_grid_res_2(mv):
    svo = build(mv, [(0, 0, 0)], 2)
    assert svo.dilation_cells_device(M.FACES) == 3 and svo.dilation_cells_device(M.CUBE) == 7
    assert_all(mv, [(0, 0, 0)], 2)
    assert_all(mv, [(1, 1, 1), (0, 1, 0)], 2, steps=(1, 2))


def test_full_grid_changes_nothing_and_keeps_the_view_valid(mv):
    svo = build(mv, full(2), 2)
    view, before, info, allocs = bytes(svo.device_view()), octree(svo), bytes(svo.info()), mv.allocation_state()[:2]
    for e in ELEMENTS:
        assert svo.dilation_cells_device(e) == 0 and svo.erosion_voxels_device(e) == 0
        assert len(svo.dilation_cells(e)["xyz"]) == 0 and len(svo.erosion_voxels(e)) == 0
        for op in OPS:
            assert getattr(svo, op)(e, 3) == 0
    assert bytes(svo.device_view()) == view and bytes(svo.info()) == info and same(octree(svo), before)
    assert mv.allocation_state()[:2] == allocs  # the same arrays at the same addresses: no rebuild


def test_centre_voxel(mv):
    svo = build(mv, [(2, 2, 2)], 4)
    assert svo.dilation_cells_device(M.FACES) == 6 and svo.dilation_cells_device(M.CUBE) == 26
    assert_listings(svo, 4)
    before, info = octree(svo), bytes(svo.info())
    for e in ELEMENTS:
        for call in (svo.erode, svo.open):
            with pytest.raises(mv.MvrtError, match="would leave no voxel"):
                call(e, 1)
            assert bytes(svo.info()) == info and same(octree(svo), before)
    assert_all(mv, [(2, 2, 2)], 4, steps=(1, 2))


def test_across_the_top_octant_seam_with_a_cell_two_voxels_reach(mv):
    xyz = [(3, 3, 3), (4, 4, 4)]
    at = np.array([[10, 20, 30, 1, 40, 50, 60, 2], [13, 21, 35, 3, 41, 53, 61, 4]], np.uint8)
    svo = build(mv, xyz, 8, attribs=at)
    cells = svo.dilation_cells(M.CUBE)
    i = int(np.flatnonzero((cells["xyz"] == (3, 3, 4)).all(1))[0])
    assert cells["count"][i] == 2 and list(cells["attribs"][i]) == [11, 20, 32, 255, 40, 51, 60, 255]  # the floors of the means of two
    assert sorted(np.bincount(cells["count"]).tolist()) == [0, 6, 38] and len(svo.dilation_cells(M.FACES)["xyz"]) == 12
    assert_all(mv, xyz, 8, attribs=at, steps=(1, 2))


def test_mean_of_26_distinct_colours_is_floored(mv):
    xyz = np.array([p for p in itertools.product(range(2, 5), repeat=3) if p != (3, 3, 3)])
    rng = np.random.default_rng(26)
    at = np.zeros((26, 8), np.uint8)
    for k in (0, 1, 2, 4, 5, 6):
        at[:, k] = rng.permutation(256)[:26]
    at[:, 3], at[:, 7] = 7, 9
    svo = build(mv, xyz, 8, attribs=at)
    x0, a0 = svo.read_voxels()
    cells = svo.dilation_cells(M.CUBE)
    i = int(np.flatnonzero((cells["xyz"] == 3).all(1))[0])
    sums = a0.astype(np.int64).sum(0)
    assert cells["count"][i] == 26 and any(sums[k] % 26 for k in (0, 1, 2, 4, 5, 6))
    assert list(cells["attribs"][i]) == [sums[0] // 26, sums[1] // 26, sums[2] // 26, 255, sums[4] // 26, sums[5] // 26, sums[6] // 26, 255]
    assert_listings(svo, 8)
    closed = assert_op(mv, xyz, 8, "close", M.CUBE, 1, attribs=at)  # the hole is plugged with that mean, nothing else stays
    assert closed.info().numberOfVoxels == 27


# ---- the run expansion: partial groups, and a group without records between two with ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_rows_with_every_second_cell_empty(mv, n):
    xyz = np.stack([np.arange(n) * 2, np.full(n, 5), np.full(n, 9)], 1)
    svo = build(mv, xyz, 2048)
    assert svo.dilation_cells_device(M.FACES) == 5 * n
    assert_listings(svo, 2048)
    for e in ELEMENTS:
        assert_op(mv, xyz, 2048, "dilate", e, 2)
        assert_op(mv, xyz, 2048, "close", e, 1)


def test_a_group_without_records_between_two_with(mv):
    """a solid 32^3 block: its sorted list holds whole 8^3 sub-blocks of interior voxels, 512 consecutive entries without an empty neighbour, 256-aligned"""
    xyz = full(32) + 32
    svo = build(mv, xyz, 128, attribs=colours(len(xyz), 3))
    for e in ELEMENTS:
        has = np.zeros(len(xyz), bool)
        has[svo.erosion_voxels(e)] = True
        groups = has.reshape(-1, 256).any(1)
        assert any(groups[g - 1] and not groups[g] and groups[g + 1:].any() for g in range(1, len(groups) - 1))
    assert_listings(svo, 128)
    assert_op(mv, xyz, 128, "dilate", M.CUBE, 1, attribs=colours(len(xyz), 3))
    assert_op(mv, xyz, 128, "open", M.FACES, 2, attribs=colours(len(xyz), 3))


# ---- the 21-bit edge -------------------------------------------------------------------------------------------------------------------------------------------
def test_borders_and_corners_of_the_largest_grid(mv):
    res = 1 << 21
    m, c = res - 1, res // 2
    xyz = [(0, c, c), (m, c, c), (c, 0, c), (c, m, c), (c, c, 0), (c, c, m)] + list(itertools.product((0, m), repeat=3))
    svo = build(mv, xyz, res)
    assert svo.info().levels == 21
    assert svo.dilation_cells_device(M.FACES) == 6 * 5 + 8 * 3 and svo.dilation_cells_device(M.CUBE) == 6 * 17 + 8 * 7  # clipped, nothing wraps
    assert_listings(svo, res, sparse=True)
    for op, e in (("dilate", M.FACES), ("dilate", M.CUBE), ("close", M.CUBE), ("close", M.FACES)):
        assert_op(mv, xyz, res, op, e, 2, sparse=True)
    # erosion does not peel at the border: of a 2 x 2 x 2 block in the far corner the corner voxel has every in-grid neighbour
    block = full(2) + (res - 2)
    for e, left in ((M.CUBE, 1), (M.FACES, 1)):
        svo = assert_op(mv, block, res, "erode", e, 1, sparse=True)
        assert svo.info().numberOfVoxels == left and svo.read_voxels()[0].tolist() == [[m, m, m]]
    assert assert_op(mv, block, res, "open", M.CUBE, 1, sparse=True).info().numberOfVoxels == 8


# ---- several steps, closing and opening ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed():
    # a block with three one-voxel holes, so that three erosion steps leave something, among specks that an opening removes
    return specks_and_block([(1, 1, 1), (10, 10, 1), (1, 10, 10)])


def unique(xyz):
    return S.sorted_voxels(xyz)


@pytest.mark.parametrize("e", ELEMENTS)
def test_three_steps_in_one_call_equal_three_calls(mv, mixed, e):
    xyz = unique(mixed)
    for op in ("dilate", "erode"):
        a, b = build(mv, xyz, 32), build(mv, xyz, 32)
        n = getattr(a, op)(e, 3)
        assert n == sum(getattr(b, op)(e, 1) for _ in range(3)) and n > 0
        assert_same_octree(a, b)
    a, b = build(mv, xyz, 32), build(mv, xyz, 32)
    added = a.close(e, 2)
    grown = b.dilate(e, 1) + b.dilate(e, 1)
    assert added == grown - b.erode(e, 1) - b.erode(e, 1)
    assert_same_octree(a, b)


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("e", ELEMENTS)
def test_close_and_open_against_the_model(mv, mixed, e, k):
    xyz = unique(mixed)
    at = colours(len(xyz), 5)
    x0, a0 = build(mv, xyz, 32, attribs=at).read_voxels()
    codes = S.morton(x0)
    closed = assert_op(mv, xyz, 32, "close", e, k, attribs=at)
    cx, ca = closed.read_voxels()
    was = np.isin(S.morton(cx), codes)
    assert was.sum() == len(x0) and np.array_equal(ca[was], a0) and (ca[~was][:, [3, 7]] == 255).all()  # a superset, the original bytes intact
    opened = assert_op(mv, xyz, 32, "open", e, k, attribs=at)
    ox, oa = opened.read_voxels()
    kept = np.isin(codes, S.morton(ox))
    assert kept.sum() == len(ox) and np.array_equal(oa, a0[kept])  # a subset with the original bytes
    # both idempotent
    assert closed.close(e, k) == 0 and 0 < len(ox) < len(x0) and opened.open(e, k) == 0


def test_in_place_calls_equal_an_edit_with_the_listing(mv, mixed):
    xyz = unique(mixed)
    at = colours(len(xyz), 6, emission=False)
    for flags, e in itertools.product((0, 3), ELEMENTS):
        a, b = build(mv, xyz, 32, flags, at), build(mv, xyz, 32, flags, at)
        for h in (a, b):
            h.set_emission_scale(3.25)
        cells = b.dilation_cells(e)
        assert a.dilate(e, 1) == len(cells["xyz"]) > 0
        b.edit_voxels(cells["xyz"], cells["attribs"])
        assert_same_octree(a, b)
        x1, _ = b.read_voxels()
        gone = b.erosion_voxels(e)
        assert a.erode(e, 1) == len(gone) > 0
        b.edit_voxels(x1[gone], None, np.zeros(len(gone), np.uint8))
        assert_same_octree(a, b)
    # an emissive source turns the flag on in the new cells' set, an erosion that removes it turns it off
    glow = at.copy()
    glow[0, 4] = 200
    a = build(mv, xyz, 32, 0, glow)
    x0, _ = a.read_voxels()
    assert a.info().hasEmission == 1
    for op, e, k in (("dilate", M.CUBE, 1), ("open", M.CUBE, 1), ("erode", M.FACES, 1)):
        assert_op(mv, xyz, 32, op, e, k, attribs=glow)


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_every_flavour(mv, mixed, flags):
    xyz = unique(mixed)
    svo = build(mv, xyz, 32, flags)
    assert flags != 3 or svo.info().flavour == 2  # the tree flavour
    assert_listings(svo, 32)
    for op in OPS:
        after = assert_op(mv, xyz, 32, op, M.CUBE, 1, flags)
        assert after.info().flavour == svo.info().flavour


def test_after_an_edit_after_a_fill_and_after_a_rebuild(mv):
    xyz = holed_shell()
    svo = build(mv, xyz, 16)
    svo.edit_voxels(np.array([(7, 7, 10), (1, 1, 1)], np.uint32), colours(2, 8))
    svo.edit_voxels(np.array([(4, 4, 4)], np.uint32), None, np.zeros(1, np.uint8))
    assert_listings(svo, 16)
    assert svo.fill_enclosed() == 125
    assert_listings(svo, 16)
    x0, a0 = svo.read_voxels()
    nodes, attrs, _ = svo.download()
    i = svo.info()
    up = mv.IntersectorOctreeGPU()
    up.upload(nodes, attrs, LOWER, DPS, 16, i.hasEmission, embeddedMask=bool(i.embeddedMask))
    for call in (up.dilation_cells_device, up.erosion_voxels_device, up.dilate, up.erode, up.close, up.open):
        with pytest.raises(mv.MvrtError, match="keeps no Morton codes"):
            call()
    up.rebuild()
    assert_listings(up, 16)
    assert up.open(M.CUBE, 1) == len(x0) - len(M.morph("open", x0, a0, 16, M.CUBE, 1)[0]) > 0
    assert same(up.read_voxels(), M.morph("open", x0, a0, 16, M.CUBE, 1))


def test_faces_erosion_equals_the_surface_masks_inside_the_grid(mv, mixed):
    xyz = np.concatenate([unique(mixed), full(4) * [1, 1, 1] + [28, 0, 14]])  # and a block on two borders of the grid
    svo = build(mv, unique(xyz), 32)
    x0, _ = svo.read_voxels()
    masks, _ = svo.surface_masks()
    x, y, z = x0[:, 0].astype(np.int64), x0[:, 1].astype(np.int64), x0[:, 2].astype(np.int64)
    outside = ((y == 0) * 1 | (y == 31) * 2 | (z == 0) * 4 | (x == 31) * 8 | (z == 31) * 16 | (x == 0) * 32).astype(np.uint8)  # d = 0 -Y, 1 +Y, 2 -Z, 3 +X, 4 +Z, 5 -X
    assert outside.any()
    assert np.array_equal(svo.erosion_voxels(M.FACES), np.flatnonzero(masks & ~outside))


def test_holed_shell_end_to_end(mv):
    svo = build(mv, holed_shell(), 16)
    assert svo.enclosed_cells_device() == (0, 0)
    faces = build(mv, holed_shell(), 16)
    assert faces.close(M.FACES, 1) == 44 and faces.enclosed_cells_device() == (0, 0)  # concave corners, the hole still open
    assert svo.close(M.CUBE, 1) == 1
    assert svo.enclosed_cells_device() == (125, 1)
    assert svo.fill_enclosed() == 125 and svo.info().numberOfVoxels == 343


def test_bunny_at_128(mv):
    tris = bunny_tris()
    v = tris.reshape(-1, 3)
    lo = v.min(0)
    dps = np.float32((v.max(0) - lo).max() / np.float32(128))
    base = mv.IntersectorOctreeGPU()
    base.build(v, None, None, None, lo, dps, 128)
    x0, a0 = base.read_voxels()
    assert len(x0) == 33487
    a0 = colours(len(x0), 12)
    for e in ELEMENTS:
        for op, k in (("close", 2), ("open", 1)):
            svo = mv.IntersectorOctreeGPU()
            svo.build_voxels(x0, a0, origin=lo, dps=dps, gridRes=128)
            a1 = svo.read_voxels()[1]
            wx, wa = M.morph(op, x0, a1, 128, e, k)
            if len(wx) == 0:  # the opening of a one-voxel shell: with FACES the few voxels the grid border backs are left, with CUBE none, which is refused
                assert (op, e) == ("open", M.CUBE)
                with pytest.raises(mv.MvrtError, match="would leave no voxel"):
                    svo.open(e, k)
                assert same(svo.read_voxels(), (x0, a1))
                continue
            n = getattr(svo, op)(e, k)
            print("bunny", op, "element", e, "steps", k, len(x0), "->", len(wx), "returned", n)
            assert n == abs(len(wx) - len(x0)) > 0 and len(wx) > 0 and same(svo.read_voxels(), (wx, wa))


def test_through_the_path_tracers_intersector_with_steps_in_flight(mv):
    """The same two steps around a closing and around the edit it stands for: the step issued before finishes first on the old octree, the frame buffer is not
    cleared, and the second step accumulates on it."""
    tris = bunny_tris()
    v = tris.reshape(-1, 3)
    lo = v.min(0)
    res, w, h = 64, 64, 36
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
        wx, wa = M.morph("dilate", x0, a0, res, M.FACES, 1)
        new = ~np.isin(S.morton(wx), S.morton(x0))
        pt.step(None, cam)
        if use_call:
            assert svo.dilate(M.FACES, 1) == new.sum()
        else:
            svo.edit_voxels(wx[new], wa[new])
        assert svo.info().numberOfVoxels == len(wx)
        pt.step(None, cam)
        assert pt.getSteps() == 2
        frames.append(pt.read_framebuffer()[: w * h].copy())
        pt.cleanUp()
    assert np.array_equal(frames[0].view(np.uint32), frames[1].view(np.uint32))


# ---- the contract ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(mv, mixed):
    return build(mv, unique(mixed), 32)


def test_null_outputs_and_capacity(mv, small):
    svo = small
    x0, a0 = svo.read_voxels()
    want = M.dilation_cells(x0, a0, 32, M.CUBE)
    n = len(want["xyz"])
    xyz, at, cnt = mv.DeviceArray((n, 3), np.uint32), mv.DeviceArray((n, 8), np.uint8), mv.DeviceArray(n, np.uint32)
    assert svo.dilation_cells_device(M.CUBE, n, xyz, None, None) == n and np.array_equal(xyz.to_host(), want["xyz"])
    assert svo.dilation_cells_device(M.CUBE, n, None, at, None) == n and np.array_equal(at.to_host(), want["attribs"])
    assert svo.dilation_cells_device(M.CUBE, n, None, None, cnt) == n and np.array_equal(cnt.to_host(), want["count"])
    lib = mv.lib()
    assert lib.mvrt_svo_dilation_cells(svo._h, M.CUBE, 0, None, None, None, None, None) == 0  # even the count may be NULL
    assert lib.mvrt_svo_erosion_voxels(svo._h, M.CUBE, 0, None, None, None) == 0
    one = build(mv, [(1, 1, 1)], 4)
    assert lib.mvrt_svo_dilate(one._h, M.CUBE, 1, None, None) == 0 and one.info().numberOfVoxels == 27
    big, host = filled(mv, (n + 5, 3), np.uint32)  # a larger capacity writes the count's worth
    assert svo.dilation_cells_device(M.CUBE, n + 5, big, None, None) == n
    assert np.array_equal(big.to_host()[:n], want["xyz"]) and np.array_equal(big.to_host()[n:], host[n:])
    # one short: the count is still returned and nothing is written
    (xyz, xyz_host), (cnt, cnt_host) = filled(mv, (n, 3), np.uint32), filled(mv, n, np.uint32)
    nc = C.c_uint64(0)
    assert lib.mvrt_svo_dilation_cells(svo._h, M.CUBE, n - 1, xyz.ptr, None, cnt.ptr, C.byref(nc), None) != 0
    assert nc.value == n and b"capacity %d" % (n - 1) in lib.mvrt_last_error() and b"%d cells" % n in lib.mvrt_last_error()
    assert np.array_equal(xyz.to_host(), xyz_host) and np.array_equal(cnt.to_host(), cnt_host)
    gone = M.erosion_voxels(x0, 32, M.FACES)
    vi, vi_host = filled(mv, len(gone), np.uint32)
    nc.value = 0
    assert lib.mvrt_svo_erosion_voxels(svo._h, M.FACES, len(gone) - 1, vi.ptr, C.byref(nc), None) != 0
    assert nc.value == len(gone) and b"capacity" in lib.mvrt_last_error() and np.array_equal(vi.to_host(), vi_host)


def test_refusals_without_gpu_work(mv, small):
    svo = small
    empty = mv.IntersectorOctreeGPU()
    nodes, attrs, _ = svo.download()
    i = svo.info()
    up = mv.IntersectorOctreeGPU()
    up.upload(nodes, attrs, LOWER, DPS, 32, i.hasEmission, embeddedMask=bool(i.embeddedMask))
    info, before = bytes(svo.info()), octree(svo)
    allocs = mv.allocation_state()[2]
    for h, text in ((empty, "no octree"), (up, "keeps no Morton codes")):
        for call in (h.dilation_cells_device, h.erosion_voxels_device, h.dilate, h.erode, h.close, h.open):
            with pytest.raises(mv.MvrtError, match=text):
                call()
    for call in (svo.dilation_cells_device, svo.erosion_voxels_device, svo.dilate, svo.erode, svo.close, svo.open):
        for e in (-1, 2):
            with pytest.raises(mv.MvrtError, match="unknown element"):
                call(e)
    for call in (svo.dilate, svo.erode, svo.close, svo.open):
        for k in (0, 65, -3):
            with pytest.raises(mv.MvrtError, match=r"steps -?\d+ is outside \[1, 64\]"):
                call(M.CUBE, k)
    assert mv.allocation_state()[2] == allocs  # on the host, before any GPU work
    assert bytes(svo.info()) == info and same(octree(svo), before)


def test_the_listings_do_not_modify_the_handle(mv, small):
    svo = small
    before, info, held = octree(svo), bytes(svo.info()), mv.allocation_state()[:2]
    assert_listings(svo, 32)
    assert bytes(svo.info()) == info and same(octree(svo), before)
    assert mv.allocation_state()[:2] == held  # the scratch is gone


def test_sixty_four_steps_build_the_levels_once(mv):
    """a voxel in a 16^3 grid: 64 dilation steps fill the grid after 45 and stop there; one build of the levels, which the allocation count shows"""
    svo = build(mv, [(0, 0, 0)], 16)
    assert svo.dilate(M.FACES, 64) == 4095 and svo.info().numberOfVoxels == 4096
    a, b = build(mv, [(3, 9, 4)], 16), build(mv, [(3, 9, 4)], 16)
    start = mv.allocation_state()[2]
    a.dilate(M.CUBE, 4)
    one = mv.allocation_state()[2] - start
    for _ in range(4):
        b.dilate(M.CUBE, 1)
    four = mv.allocation_state()[2] - start - one
    print("allocations: one 4-step call", one, "four 1-step calls", four)
    assert_same_octree(a, b)
    assert one < four
