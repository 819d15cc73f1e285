"""Round offsets on the GPU (mvrt_svo_distance_cells / _depth_voxels / _dilate_ball / _erode_ball / _close_ball / _open_ball) against the numpy model of
tests/ball_expected.py, bit for bit: the listings array by array, the in-place calls through read_voxels, the identity with the edit through download() of a
second handle that was given the listing via edit_voxels.  On the smallest inputs that can break each mechanism -- a corner voxel and the full grid at gridRes 2,
a centre voxel at the radii where the reach changes and where it does not, two voxels with an equidistant cell between them, a pair across the top octant seam,
the borders and corners of the 2^21 grid, rows of 255 to 513 voxels with every second cell empty, a solid 17^3 block, the full reach of 32 on one voxel, the holed
shell and a whisker, every flavour, edits, fills, a rebuilt upload, steps in flight, the bunny -- and the contract of the six calls.  The count limits (a pass
whose records or a dilation whose voxels would reach 2^32 - 1) are host comparisons (csrc/kernels_ball.hip) covered by reading: reaching them takes 2^32 entries."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import ball_expected as B
import morph_expected as M
import surface_expected as S
from common import GOLDEN, bunny_tris, probe_camera
from fixtures import mv  # noqa: F401 (fixtures)
from voxel_sets import DPS, LOWER, assert_same_octree, build, colours, filled, full, holed_shell, octree, same, specks_and_block

pytestmark = pytest.mark.gpu

OPS = ("dilate", "erode", "close", "open")


def assert_listings(svo, res, rho, sparse=False):
    x0, a0 = svo.read_voxels()
    want, got = B.distance_cells(x0, a0, res, rho, sparse), svo.distance_cells(rho)
    n = len(want["xyz"])
    print("rho", rho, "distance cells", len(got["xyz"]), "model", n)
    assert svo.distance_cells_device(rho) == n  # the sizing call
    assert got["xyz"].shape == (n, 3) and got["xyz"].dtype == np.uint32 and np.array_equal(got["xyz"], want["xyz"])
    assert got["dist2"].dtype == np.uint32 and np.array_equal(got["dist2"], want["dist2"])
    assert got["nearest"].dtype == np.uint32 and np.array_equal(got["nearest"], want["nearest"])
    assert got["attribs"].shape == (n, 8) and np.array_equal(got["attribs"], want["attribs"])
    want, got = B.depth_voxels(x0, res, rho, sparse), svo.depth_voxels(rho)
    print("rho", rho, "depth voxels", len(got["vIndex"]), "model", len(want["vIndex"]))
    assert svo.depth_voxels_device(rho) == len(want["vIndex"])
    assert got["vIndex"].dtype == np.uint32 and np.array_equal(got["vIndex"], want["vIndex"]) and np.array_equal(got["depth2"], want["depth2"])
    return n


def assert_op(mv, xyz, res, op, rho, flags=0, attribs=None, sparse=False):
    """one in-place call on a fresh build against the model; a call that would leave no voxel is refused with the handle byte-identical"""
    svo = build(mv, xyz, res, flags, attribs)
    x0, a0 = svo.read_voxels()
    wx, wa = B.ball(op, x0, a0, res, rho, sparse)
    before, info = octree(svo), bytes(svo.info())
    call = getattr(svo, op + "_ball")
    if len(wx) == 0:
        with pytest.raises(mv.MvrtError, match="would leave no voxel"):
            call(rho)
        assert bytes(svo.info()) == info and same(octree(svo), before)
        return svo
    n = call(rho)
    gx, ga = svo.read_voxels()
    print(op, "rho", rho, "voxels", len(x0), "->", len(gx), "model", len(wx), "returned", n)
    assert n == abs(len(wx) - len(x0)) and svo.info().numberOfVoxels == len(wx)
    assert np.array_equal(gx, wx) and np.array_equal(ga, wa)
    assert svo.info().hasEmission == int(wa[:, 4:7].any())
    if n == 0:
        assert bytes(svo.info()) == info and same(octree(svo), before)
    return svo


def assert_all(mv, xyz, res, rhos, flags=0, attribs=None, sparse=False):
    svo = build(mv, xyz, res, flags, attribs)
    for rho in rhos:
        assert_listings(svo, res, rho, sparse)
        for op in OPS:
            assert_op(mv, xyz, res, op, rho, flags, attribs, sparse)


# ---- the smallest grids ----------------------------------------------------------------------------------------------------------------------------------------
def test_corner_voxel_at_grid_res_2(mv):
    svo = build(mv, [(0, 0, 0)], 2)
    assert [svo.distance_cells_device(rho) for rho in (1, 2, 3)] == [3, 6, 7]
    assert_all(mv, [(0, 0, 0)], 2, (1, 2, 3))
    assert_all(mv, [(1, 1, 1), (0, 1, 0)], 2, (1, 2, 3))


def test_full_grid_changes_nothing_and_keeps_the_view_valid(mv):
    svo = build(mv, full(2), 2)
    view, before, info, allocs = bytes(svo.device_view()), octree(svo), bytes(svo.info()), mv.allocation_state()[:2]
    for rho in (1, 3, 1024):
        assert svo.distance_cells_device(rho) == 0 and svo.depth_voxels_device(rho) == 0
        assert len(svo.distance_cells(rho)["xyz"]) == 0 and len(svo.depth_voxels(rho)["vIndex"]) == 0
        for op in OPS:
            assert getattr(svo, op + "_ball")(rho) == 0
    assert bytes(svo.device_view()) == view and bytes(svo.info()) == info and same(octree(svo), before)
    assert mv.allocation_state()[:2] == allocs  # the same arrays at the same addresses: no rebuild


@pytest.mark.parametrize("rho", [1, 2, 3, 4, 5, 8, 9])
def test_centre_voxel_adds_the_ball(mv, rho):
    svo = build(mv, [(16, 16, 16)], 32)
    assert assert_listings(svo, 32, rho) == len(B.ball_offsets(rho)[1]) - 1 == {1: 6, 2: 18, 3: 26, 4: 32, 5: 56, 8: 92, 9: 122}[rho]
    before, info = octree(svo), bytes(svo.info())
    for call in (svo.erode_ball, svo.open_ball):
        with pytest.raises(mv.MvrtError, match="would leave no voxel"):
            call(rho)
        assert bytes(svo.info()) == info and same(octree(svo), before)
    assert_op(mv, [(16, 16, 16)], 32, "dilate", rho)
    assert assert_op(mv, [(16, 16, 16)], 32, "close", rho).info().numberOfVoxels == 1  # the ball erodes back to its centre


@pytest.mark.parametrize("b", [(10, 8, 8), (11, 9, 8), (12, 8, 8)])
def test_a_tie_goes_to_the_lower_vindex_and_shows_in_the_attribute(mv, b):
    """two voxels 2, 3 and 4 cells apart along x.  Three apart, no cell of the axis is equidistant (the bisecting plane lies between two cells); one cell of offset
    in y puts (9, 10, 8) at squared distance 5 from both."""
    a = (8, 8, 8)  # vIndex is the Morton rank: a comes first
    at = np.array([[200, 210, 220, 3, 41, 53, 61, 4], [10, 20, 30, 1, 40, 50, 60, 2]], np.uint8)
    svo = build(mv, [b, a], 32, attribs=at)
    assert svo.read_voxels()[0].tolist() == [list(a), list(b)]
    cells = svo.distance_cells(5)
    c = cells["xyz"].astype(np.int64)
    da, db = ((c - a) ** 2).sum(1), ((c - b) ** 2).sum(1)
    tie = da == db
    print("b", b, "cells", len(c), "equidistant", int(tie.sum()))
    assert tie.any() and (cells["nearest"][tie] == 0).all() and (cells["attribs"][tie] == [10, 20, 30, 255, 40, 50, 60, 255]).all()
    assert (cells["nearest"][da < db] == 0).all() and (cells["nearest"][db < da] == 1).all() and (db < da).any()
    assert (cells["attribs"][db < da] == [200, 210, 220, 255, 41, 53, 61, 255]).all() and np.array_equal(cells["dist2"], np.minimum(da, db))
    assert_listings(svo, 32, 5)
    for op in ("dilate", "close"):
        assert_op(mv, [b, a], 32, op, 5, attribs=at)


def test_across_the_top_octant_seam(mv):
    xyz = [(15, 7, 9), (16, 7, 9)]  # x = R / 2 - 1 and R / 2: their codes differ in the top bit group
    assert_all(mv, xyz, 32, (1, 2, 5, 9), attribs=colours(2, 4))
    assert_all(mv, [(15, 15, 15), (16, 16, 16)], 32, (3, 4))


def test_borders_and_corners_of_the_largest_grid(mv):
    res = 1 << 21
    m, c = res - 1, res // 2
    xyz = [(0, c, c), (m, c, c), (c, 0, c), (c, m, c), (c, c, 0), (c, c, m)] + list(itertools.product((0, m), repeat=3))
    svo = build(mv, xyz, res)
    assert svo.info().levels == 21
    assert svo.distance_cells_device(1) == 6 * 5 + 8 * 3 and svo.distance_cells_device(3) == 6 * 17 + 8 * 7  # clipped, nothing wraps
    for rho in (1, 4, 9):
        assert_listings(svo, res, rho, sparse=True)
    for op, rho in (("dilate", 2), ("dilate", 9), ("close", 5)):
        assert_op(mv, xyz, res, op, rho, sparse=True)
    # erosion does not peel at the border: of a 3 x 3 x 3 block in the far corner the voxels the border backs stay
    block = full(3) + (res - 3)
    svo = assert_op(mv, block, res, "erode", 1, sparse=True)
    assert svo.info().numberOfVoxels == 8
    svo = assert_op(mv, block, res, "erode", 4, sparse=True)
    assert svo.read_voxels()[0].tolist() == [[m, m, m]]
    assert assert_op(mv, block, res, "open", 2, sparse=True).info().numberOfVoxels == 26  # the 2^3 corner grown again: all but (m - 2, m - 2, m - 2)


# ---- the run expansion: partial groups, groups without records, items of several chunks -----------------------------------------------------------------------
@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_rows_with_every_second_cell_empty(mv, n):
    xyz = np.stack([np.arange(n) * 2, np.full(n, 5), np.full(n, 9)], 1)
    svo = build(mv, xyz, 2048)
    assert svo.distance_cells_device(1) == 5 * n
    for rho in (1, 5):
        assert_listings(svo, 2048, rho)
    assert_op(mv, xyz, 2048, "dilate", 4)
    assert_op(mv, xyz, 2048, "close", 2)


def test_a_solid_block(mv):
    """a solid 17^3 block: stretches of interior voxels without a seed, and with rho = 16 groups of 256 entries whose records (up to 9 each) fill more than one
    turn of the workgroup"""
    xyz = full(17) + 20
    at = colours(len(xyz), 3)
    svo = build(mv, xyz, 64, attribs=at)
    for rho in (1, 6, 16):
        assert_listings(svo, 64, rho)
    assert_op(mv, xyz, 64, "dilate", 16, attribs=at)
    eroded = assert_op(mv, xyz, 64, "erode", 9, attribs=at)
    assert eroded.info().numberOfVoxels == 11 ** 3
    assert assert_op(mv, xyz, 64, "open", 6, attribs=at).info().numberOfVoxels < 17 ** 3  # the corners are rounded off


def test_the_full_reach_on_one_voxel(mv):
    """rho = 1024: 65 shifts per entry in every pass"""
    svo = build(mv, [(64, 64, 64)], 128)
    n = assert_listings(svo, 128, 1024, sparse=True)
    assert n == len(B.ball_offsets(1024)[1]) - 1
    stats = mv.ball_stats()  # of the depth listing, the last band: 6 seeds
    assert stats["seeds"] == 6 and stats["records"][0] > 6 * 60
    assert_op(mv, [(64, 64, 64)], 128, "dilate", 1024, sparse=True)


# ---- closing and opening -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed():
    return S.sorted_voxels(specks_and_block([(1, 1, 1), (10, 10, 1), (1, 10, 10)]))  # a block with three one-voxel holes among specks that an opening removes


@pytest.mark.parametrize("rho", [1, 2, 5, 9])
def test_close_and_open_against_the_model(mv, mixed, rho):
    xyz = mixed
    at = colours(len(xyz), 5)
    x0, a0 = build(mv, xyz, 32, attribs=at).read_voxels()
    codes = S.morton(x0)
    closed = assert_op(mv, xyz, 32, "close", rho, attribs=at)
    cx, ca = closed.read_voxels()
    was = np.isin(S.morton(cx), codes)
    assert was.sum() == len(x0) and np.array_equal(ca[was], a0) and (ca[~was][:, [3, 7]] == 255).all()  # a superset, the original bytes intact
    opened = assert_op(mv, xyz, 32, "open", rho, attribs=at)
    ox, oa = opened.read_voxels()
    kept = np.isin(codes, S.morton(ox))
    assert kept.sum() == len(ox) and np.array_equal(oa, a0[kept])  # a subset with the original bytes
    assert closed.close_ball(rho) == 0 and 0 < len(ox) < len(x0) and opened.open_ball(rho) == 0  # both idempotent
    assert_listings(closed, 32, rho)


def test_as_sets_a_ball_of_1_and_3_is_a_faces_and_a_cube_step(mv, mixed):
    for rho, e in ((1, M.FACES), (3, M.CUBE)):
        for op in ("dilate", "erode"):
            a, b = build(mv, mixed, 32), build(mv, mixed, 32)
            assert getattr(a, op + "_ball")(rho) == getattr(b, op)(e, 1) > 0
            assert np.array_equal(a.read_voxels()[0], b.read_voxels()[0])


def test_in_place_calls_equal_an_edit_with_the_listing(mv, mixed):
    xyz = mixed
    at = colours(len(xyz), 6, emission=False)
    for flags, rho in itertools.product((0, 3), (2, 5)):
        a, b = build(mv, xyz, 32, flags, at), build(mv, xyz, 32, flags, at)
        for h in (a, b):
            h.set_emission_scale(3.25)
        cells = b.distance_cells(rho)
        assert a.dilate_ball(rho) == len(cells["xyz"]) > 0
        b.edit_voxels(cells["xyz"], cells["attribs"])
        assert_same_octree(a, b)
        x1, _ = b.read_voxels()
        gone = b.depth_voxels(rho)["vIndex"]
        assert a.erode_ball(rho) == len(gone) > 0
        b.edit_voxels(x1[gone], None, np.zeros(len(gone), np.uint8))
        assert_same_octree(a, b)
    # hasEmission is recomputed: an emissive source turns the flag on in the set of the new cells, an erosion that removes it turns it off
    glow = at.copy()
    glow[0, 4] = 200
    assert build(mv, xyz, 32, 0, glow).info().hasEmission == 1
    flags_seen = {assert_op(mv, xyz, 32, op, rho, attribs=glow).info().hasEmission for op, rho in (("dilate", 3), ("open", 3), ("erode", 1), ("close", 4))}
    assert flags_seen == {0, 1}


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_every_flavour(mv, mixed, flags):
    svo = build(mv, mixed, 32, flags)
    assert flags != 3 or svo.info().flavour == 2  # the tree flavour
    assert_listings(svo, 32, 5)
    for op in OPS:
        after = assert_op(mv, mixed, 32, op, 4, flags)
        assert after.info().flavour == svo.info().flavour


def test_after_an_edit_after_a_fill_and_after_a_rebuild(mv):
    svo = build(mv, holed_shell(), 16)
    svo.edit_voxels(np.array([(7, 7, 10), (1, 1, 1)], np.uint32), colours(2, 8))
    svo.edit_voxels(np.array([(4, 4, 4)], np.uint32), None, np.zeros(1, np.uint8))
    assert_listings(svo, 16, 5)
    assert svo.fill_enclosed() == 125
    assert_listings(svo, 16, 5)
    x0, a0 = svo.read_voxels()
    nodes, attrs, _ = svo.download()
    i = svo.info()
    up = mv.IntersectorOctreeGPU()
    up.upload(nodes, attrs, LOWER, DPS, 16, i.hasEmission, embeddedMask=bool(i.embeddedMask))
    for call in (up.distance_cells_device, up.depth_voxels_device, up.dilate_ball, up.erode_ball, up.close_ball, up.open_ball):
        with pytest.raises(mv.MvrtError, match="keeps no Morton codes"):
            call()
    up.rebuild()
    assert_listings(up, 16, 5)
    want = B.ball("open", x0, a0, 16, 4)
    assert up.open_ball(4) == len(x0) - len(want[0]) > 0
    assert same(up.read_voxels(), want)


def test_holed_shell_and_whisker(mv):
    svo = build(mv, holed_shell(), 16)
    assert svo.enclosed_cells_device() == (0, 0)
    assert svo.close_ball(1) == 44 and svo.enclosed_cells_device() == (0, 0)  # as the FACES closing: concave corners, the hole still open
    svo = build(mv, holed_shell(), 16)
    assert svo.close_ball(3) == 1 and svo.enclosed_cells_device() == (125, 1)  # as the CUBE closing: exactly the hole
    assert svo.fill_enclosed() == 125 and svo.info().numberOfVoxels == 343
    svo = build(mv, holed_shell(), 16)
    assert svo.close_ball(5) == 69 and svo.enclosed_cells_device() == (57, 1)  # (68 cells of the cavity and the hole)
    assert_op(mv, holed_shell(), 16, "close", 5)
    # a block with a one-voxel whisker: the opening removes the whisker alone and keeps the original bytes
    block = np.concatenate([full(7) + 4, [(11, 7, 7), (12, 7, 7), (13, 7, 7)]])
    at = colours(len(block), 9)
    opened = assert_op(mv, block, 16, "open", 3, attribs=at)  # (the ball of 3 is the 3^3 block, whose openings keep a cube whole)
    ox, oa = opened.read_voxels()
    assert len(ox) == 343 and ox.max() == 10
    x0, a0 = build(mv, block, 16, attribs=at).read_voxels()
    assert np.array_equal(oa, a0[np.isin(S.morton(x0), S.morton(ox))])


def test_bunny_at_64(mv):
    tris = bunny_tris()
    v = tris.reshape(-1, 3)
    lo = v.min(0)
    dps = np.float32((v.max(0) - lo).max() / np.float32(64))
    base = mv.IntersectorOctreeGPU()
    base.build(v, None, None, None, lo, dps, 64)
    x0, _ = base.read_voxels()
    a0 = colours(len(x0), 12)
    svo = mv.IntersectorOctreeGPU()
    svo.build_voxels(x0, a0, origin=lo, dps=dps, gridRes=64)
    a1 = svo.read_voxels()[1]
    assert_listings(svo, 64, 5)
    wx, wa = B.ball("close", x0, a1, 64, 5)
    n = svo.close_ball(5)
    print("bunny close rho 5", len(x0), "->", len(wx), "returned", n)
    assert n == len(wx) - len(x0) > 0 and same(svo.read_voxels(), (wx, wa))


def test_through_the_path_tracers_intersector_with_steps_in_flight(mv):
    """The same two steps around a ball dilation and around the edit it stands for: the step issued before finishes first on the old octree, the frame buffer is
    not cleared, and the second step accumulates on it."""
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
        wx, wa = B.ball("dilate", x0, a0, res, 2)
        new = ~np.isin(S.morton(wx), S.morton(x0))
        pt.step(None, cam)
        if use_call:
            assert svo.dilate_ball(2) == new.sum()
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
    return build(mv, mixed, 32)


def test_null_outputs_and_capacity(mv, small):
    svo = small
    x0, a0 = svo.read_voxels()
    want = B.distance_cells(x0, a0, 32, 5)
    n = len(want["xyz"])
    xyz, d2, near, at = mv.DeviceArray((n, 3), np.uint32), mv.DeviceArray(n, np.uint32), mv.DeviceArray(n, np.uint32), mv.DeviceArray((n, 8), np.uint8)
    assert svo.distance_cells_device(5, n, xyz) == n and np.array_equal(xyz.to_host(), want["xyz"])
    assert svo.distance_cells_device(5, n, None, d2) == n and np.array_equal(d2.to_host(), want["dist2"])
    assert svo.distance_cells_device(5, n, None, None, near) == n and np.array_equal(near.to_host(), want["nearest"])
    assert svo.distance_cells_device(5, n, None, None, None, at) == n and np.array_equal(at.to_host(), want["attribs"])
    lib = mv.lib()
    assert lib.mvrt_svo_distance_cells(svo._h, 5, 0, None, None, None, None, None, None) == 0  # even the count may be NULL
    assert lib.mvrt_svo_depth_voxels(svo._h, 5, 0, None, None, None, None) == 0
    one = build(mv, [(1, 1, 1)], 4)
    assert lib.mvrt_svo_dilate_ball(one._h, 3, None, None) == 0 and one.info().numberOfVoxels == 27
    big, host = filled(mv, (n + 5, 3), np.uint32)  # a larger capacity writes the count's worth
    assert svo.distance_cells_device(5, n + 5, big) == n
    assert np.array_equal(big.to_host()[:n], want["xyz"]) and np.array_equal(big.to_host()[n:], host[n:])
    # one short: the count is still returned and nothing is written
    (xyz, xyz_host), (near, near_host) = filled(mv, (n, 3), np.uint32), filled(mv, n, np.uint32)
    nc = C.c_uint64(0)
    assert lib.mvrt_svo_distance_cells(svo._h, 5, n - 1, xyz.ptr, None, near.ptr, None, C.byref(nc), None) != 0
    assert nc.value == n and b"capacity %d" % (n - 1) in lib.mvrt_last_error() and b"%d cells" % n in lib.mvrt_last_error()
    assert np.array_equal(xyz.to_host(), xyz_host) and np.array_equal(near.to_host(), near_host)
    gone = B.depth_voxels(x0, 32, 5)
    m = len(gone["vIndex"])
    vi, dp = mv.DeviceArray(m, np.uint32), mv.DeviceArray(m, np.uint32)
    assert svo.depth_voxels_device(5, m, vi, None) == m and np.array_equal(vi.to_host(), gone["vIndex"])
    assert svo.depth_voxels_device(5, m, None, dp) == m and np.array_equal(dp.to_host(), gone["depth2"])
    (vi, vi_host), (dp, dp_host) = filled(mv, m, np.uint32), filled(mv, m, np.uint32)
    nc.value = 0
    assert lib.mvrt_svo_depth_voxels(svo._h, 5, m - 1, vi.ptr, dp.ptr, C.byref(nc), None) != 0
    assert nc.value == m and b"capacity" in lib.mvrt_last_error() and np.array_equal(vi.to_host(), vi_host) and np.array_equal(dp.to_host(), dp_host)


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
        for call in (h.distance_cells_device, h.depth_voxels_device, h.dilate_ball, h.erode_ball, h.close_ball, h.open_ball):
            with pytest.raises(mv.MvrtError, match=text):
                call()
    for call in (svo.distance_cells_device, svo.depth_voxels_device, svo.dilate_ball, svo.erode_ball, svo.close_ball, svo.open_ball):
        for rho in (0, 1025, 1 << 31):
            with pytest.raises(mv.MvrtError, match=r"radius2 \d+ is outside \[1, 1024\]"):
                call(rho)
    assert mv.allocation_state()[2] == allocs  # on the host, before any GPU work
    assert bytes(svo.info()) == info and same(octree(svo), before)


def test_the_listings_do_not_modify_the_handle(mv, small):
    svo = small
    before, info, held = octree(svo), bytes(svo.info()), mv.allocation_state()[:2]
    for rho in (1, 5, 100):
        assert_listings(svo, 32, rho)
    assert bytes(svo.info()) == info and same(octree(svo), before)
    assert mv.allocation_state()[:2] == held  # the scratch is gone
    # with rho = 1024 the depth listing holds every voxel of a set that fits in the reach: a wall-thickness probe
    assert svo.depth_voxels_device(1024) == svo.info().numberOfVoxels
