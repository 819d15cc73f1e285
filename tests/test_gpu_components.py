"""Connected components on the GPU (mvrt_svo_components / mvrt_svo_keep_components) against the model of tests/components_expected.py, bit for bit: the listing
array by array, the in-place call through read_voxels, the identity with the edit through a second handle that was given the model's dropped voxels via
edit_voxels.  On the smallest inputs that can break each mechanism -- gridRes 2, two voxels across the top octant seam, the borders of the 2^21 grid, the 3-D
checkerboard (every lane of a wave its own label under FACES, one component summed over waves and workgroups under CUBE), a U whose arms merge at the highest
codes, a serpentine chain, random sets with hundreds of components and tied sizes, every flavour, edits, fills, an opening, a rebuilt upload, steps in flight, the
bunny -- and the contract of the two calls."""
import ctypes as C
import os

import numpy as np
import pytest

import components_expected as K
import surface_expected as S
from common import GOLDEN, bunny_tris, probe_camera
from fixtures import mv  # noqa: F401 (fixtures)
from voxel_sets import DPS, LOWER, assert_same_octree, build, colours, filled, full, octree, same, specks_and_block

pytestmark = pytest.mark.gpu

ELEMENTS = (K.FACES, K.CUBE)
REMOVE = 0  # IntersectorOctreeGPU.VOXEL_REMOVE


def assert_listing(svo, res, sparse=False, elements=ELEMENTS):
    """both elements against the model, array by array; returns the model's results"""
    x0, _ = svo.read_voxels()
    out = {}
    for e in elements:
        want, got = K.components(x0, res, e, sparse), svo.components(e)
        n = len(want["size"])
        print("element", e, "voxels", len(x0), "components", len(got["size"]), "model", n, "largest", got["size"].max(), "model", want["size"].max())
        assert svo.components_device(e) == (n, want["size"].max())  # the sizing call
        assert got["label"].dtype == np.uint32 and got["label"].shape == (len(x0),) and np.array_equal(got["label"], want["label"])
        assert got["size"].dtype == np.uint32 and got["size"].shape == (n,) and np.array_equal(got["size"], want["size"])
        assert got["first"].dtype == np.uint32 and np.array_equal(got["first"], want["first"])
        assert got["box"].dtype == np.uint32 and got["box"].shape == (n, 6) and np.array_equal(got["box"], want["box"])
        out[e] = want
    return out


def assert_keep(mv, xyz, res, e, min_voxels=1, keep_largest=0, flags=0, attribs=None, sparse=False, svo=None):
    """one in-place call (on a fresh build unless a handle is given) against the model and against the edit it stands for"""
    svo = build(mv, xyz, res, flags, attribs) if svo is None else svo
    x0, a0 = svo.read_voxels()
    c = K.components(x0, res, e, sparse)
    stays = K.kept_components(c["size"], min_voxels, keep_largest)
    wx, wa = K.keep(x0, a0, res, e, min_voxels, keep_largest, sparse)
    before, info = octree(svo), bytes(svo.info())
    if len(wx) == 0:
        with pytest.raises(mv.MvrtError, match="would leave no voxel"):
            svo.keep_components(e, min_voxels, keep_largest)
        assert bytes(svo.info()) == info and same(octree(svo), before)
        return svo
    twin = mv.IntersectorOctreeGPU()
    i = svo.info()
    twin.build_voxels(x0, a0, origin=np.array(i.lower[:], np.float32), dps=np.float32(i.dps), gridRes=res, flags=flags)
    twin.set_emission_scale(i.emissionScale)
    removed, kept = svo.keep_components(e, min_voxels, keep_largest)
    gx, ga = svo.read_voxels()
    print("keep element", e, "min", min_voxels, "largest", keep_largest, "voxels", len(x0), "->", len(gx), "model", len(wx), "components", len(stays), "->", kept)
    assert (removed, kept) == (len(x0) - len(wx), stays.sum()) and svo.info().numberOfVoxels == len(wx)
    assert np.array_equal(gx, wx) and np.array_equal(ga, wa)
    assert svo.info().hasEmission == int(wa[:, 4:7].any())
    if removed == 0:
        assert bytes(svo.info()) == info and same(octree(svo), before)
    else:
        gone = K.dropped(x0, res, e, min_voxels, keep_largest, sparse)
        twin.edit_voxels(gone.astype(np.uint32), None, np.full(len(gone), REMOVE, np.uint8))
        assert_same_octree(svo, twin)
    return svo


def checkerboard(res):
    return np.argwhere(np.indices((res,) * 3).sum(0) % 2 == 0)


def u_shape():
    """two arms along x at y = 2 and y = 12, joined only by a bar at x = 15, the end with the highest codes: both arms start as roots and merge late"""
    arm = np.arange(16)
    bar = np.arange(3, 12)
    return np.concatenate([np.stack([arm, np.full(16, 2), np.full(16, 3)], 1), np.stack([arm, np.full(16, 12), np.full(16, 3)], 1),
                           np.stack([np.full(len(bar), 15), bar, np.full(len(bar), 3)], 1)])


def serpentine(res=32):
    """one 6-connected path: rows along x on every second y, joined alternately at the two ends, layers on every second z joined the same way"""
    g = np.zeros((res, res, res), bool)
    for k, z in enumerate(range(0, res, 2)):
        for j, y in enumerate(range(0, res, 2)):
            g[:, y, z] = True
            if y + 2 < res:
                g[res - 1 if j % 2 == 0 else 0, y + 1, z] = True
        if z + 2 < res:  # the layers are joined at the end of their last row
            g[0, res - 2, z + 1] = True
    return np.argwhere(g)


@pytest.fixture(scope="module")
def random_sets():
    rng = np.random.default_rng(7)
    return {K.CUBE: np.argwhere(rng.random((32, 32, 32)) < 0.1), K.FACES: np.argwhere(np.random.default_rng(7).random((32, 32, 32)) < 0.3)}


# ---- the smallest grids ----------------------------------------------------------------------------------------------------------------------------------------
def test_grid_res_2(mv):
    got = assert_listing(build(mv, [(1, 0, 1)], 2), 2)
    assert all(len(got[e]["size"]) == 1 for e in ELEMENTS)
    got = assert_listing(build(mv, full(2), 2), 2)
    assert all(got[e]["size"].tolist() == [8] for e in ELEMENTS)
    for other in ((1, 1, 0), (1, 1, 1)):
        got = assert_listing(build(mv, [(0, 0, 0), other], 2), 2)
        assert got[K.FACES]["size"].tolist() == [1, 1] and got[K.CUBE]["size"].tolist() == [2]
        for e in ELEMENTS:
            assert_keep(mv, [(0, 0, 0), other], 2, e, keep_largest=1)
            assert_keep(mv, [(0, 0, 0), other], 2, e, min_voxels=2)  # under FACES: refused


def test_across_the_top_octant_seam(mv):
    xyz = [(7, 3, 3), (8, 3, 3), (7, 7, 7)]  # in Morton order the third lies between the two that are adjacent
    got = assert_listing(build(mv, xyz, 16), 16)
    for e in ELEMENTS:
        assert got[e]["label"].tolist() == [0, 1, 0] and got[e]["first"].tolist() == [0, 1]
        assert_keep(mv, xyz, 16, e, min_voxels=2)


def test_nothing_wraps_at_the_largest_grid(mv):
    R, y, z = 1 << 21, 5, 9
    xyz = [(0, y, z), (R - 1, y, z), (0, y + 1, z), (R - 1, R - 1, R - 1), (R - 2, R - 2, R - 1), (R - 1, 0, 0), (0, 1, 0)]
    svo = build(mv, xyz, R)
    assert svo.info().levels == 21
    got = assert_listing(svo, R, sparse=True)
    assert sorted(got[K.FACES]["size"].tolist()) == [1, 1, 1, 1, 1, 2] and sorted(got[K.CUBE]["size"].tolist()) == [1, 1, 1, 2, 2]
    assert_keep(mv, xyz, R, K.CUBE, min_voxels=2, sparse=True)
    assert_keep(mv, xyz, R, K.FACES, keep_largest=1, sparse=True)


# ---- the wave aggregation ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [8, 16])
def test_checkerboard(mv, res):
    xyz = checkerboard(res)
    assert len(xyz) == res ** 3 // 2
    got = assert_listing(build(mv, xyz, res), res)
    assert len(got[K.FACES]["size"]) == len(xyz) and got[K.CUBE]["size"].tolist() == [len(xyz)]
    assert_keep(mv, xyz, res, K.FACES, keep_largest=3)  # all tied: the three lowest labels
    assert_keep(mv, xyz, res, K.CUBE, keep_largest=1)  # nothing goes


# ---- the union-find ------------------------------------------------------------------------------------------------------------------------------------------------
def test_u_shape(mv):
    xyz = np.concatenate([u_shape(), [(3, 7, 3)]])  # and a speck between the arms
    got = assert_listing(build(mv, xyz, 16), 16)
    for e in ELEMENTS:
        assert sorted(got[e]["size"].tolist()) == [1, 41] and got[e]["first"][0] == 0 and got[e]["label"].max() == 1
    assert_keep(mv, xyz, 16, K.FACES, keep_largest=1)


def test_serpentine_path(mv):
    xyz = serpentine()
    svo = build(mv, xyz, 32)
    got = assert_listing(svo, 32)
    assert 2000 < len(xyz) < 10000 and got[K.FACES]["size"].tolist() == [len(xyz)] and got[K.FACES]["box"].tolist() == [[0, 0, 0, 31, 30, 30]]


@pytest.mark.parametrize("e", ELEMENTS)
def test_random_sets(mv, random_sets, e):
    xyz = random_sets[e]
    svo = build(mv, xyz, 32)
    want = assert_listing(svo, 32, elements=(e,))[e]
    sizes, counts = np.unique(want["size"], return_counts=True)
    assert len(want["size"]) >= 500 and want["size"].max() >= 256 and (counts > 1).any()
    order = np.sort(want["size"])[::-1]
    assert_keep(mv, xyz, 32, e, keep_largest=1)
    assert_keep(mv, xyz, 32, e, min_voxels=int(order[5]), keep_largest=40)  # both rules; the size rule binds
    assert_keep(mv, xyz, 32, e, min_voxels=2, keep_largest=7)  # the rank rule binds, inside a run of tied sizes or not
    tied = int(sizes[counts > 1].max())  # the largest size that two components share: cut inside that run
    above = int((want["size"] > tied).sum())
    assert_keep(mv, xyz, 32, e, keep_largest=above + 1)


# ---- keep_components -----------------------------------------------------------------------------------------------------------------------------------------------
def blocks():
    """components of 5, 8, 8, 3 and 1 voxels in a 16^3 grid, in this order of first appearance"""
    row = lambda n, y, z, x0=0: [(x0 + i, y, z) for i in range(n)]
    return np.array(row(5, 0, 0) + row(8, 4, 0) + row(8, 0, 4) + row(3, 8, 8) + row(1, 12, 12))


def test_keep_largest_and_ties(mv):
    xyz = blocks()
    got = assert_listing(build(mv, xyz, 16), 16)
    assert got[K.FACES]["size"].tolist() == [5, 8, 8, 3, 1]
    for e in ELEMENTS:
        one = assert_keep(mv, xyz, 16, e, keep_largest=1, attribs=colours(len(xyz), 4))
        assert one.read_voxels()[0].tolist() == [[i, 4, 0] for i in range(8)]  # the lower label wins
        two = assert_keep(mv, xyz, 16, e, keep_largest=2)
        assert two.info().numberOfVoxels == 16
        assert_keep(mv, xyz, 16, e, keep_largest=3)
        assert_keep(mv, xyz, 16, e, keep_largest=99)


@pytest.mark.parametrize("min_voxels", [4, 5, 6, 8, 9])
def test_min_voxels_around_a_size(mv, min_voxels):
    svo = assert_keep(mv, blocks(), 16, K.FACES, min_voxels=min_voxels, attribs=colours(25, 9, emission=False))
    assert svo.info().numberOfVoxels == {4: 21, 5: 21, 6: 16, 8: 16, 9: 25}[min_voxels]  # (9: refused, nothing changed)


def test_both_rules_together_and_emission(mv):
    xyz = blocks()
    at = colours(len(xyz), 2, emission=False)
    at[-1, 5] = 77  # only the speck glows (the last voxel in Morton order too: (0, 12, 12))
    svo = build(mv, xyz, 16, attribs=at)
    assert svo.info().hasEmission == 1 and svo.read_voxels()[1][-1, 5] == 77
    after = assert_keep(mv, xyz, 16, K.CUBE, min_voxels=4, keep_largest=2, attribs=at)
    assert after.info().hasEmission == 0 and after.info().numberOfVoxels == 16
    after = assert_keep(mv, xyz, 16, K.CUBE, min_voxels=8, keep_largest=3, attribs=at)
    assert after.info().numberOfVoxels == 16
    after = assert_keep(mv, xyz, 16, K.CUBE, min_voxels=1, keep_largest=5, attribs=at)
    assert after.info().hasEmission == 1


def test_nothing_dropped_leaves_the_handle_and_its_views(mv):
    svo = build(mv, blocks(), 16)
    view, before, info, allocs = bytes(svo.device_view()), octree(svo), bytes(svo.info()), mv.allocation_state()[:2]
    for e in ELEMENTS:
        assert svo.keep_components(e) == (0, 5)
        assert svo.keep_components(e, 1, 5) == (0, 5)
        assert svo.keep_components(e, 1, 0xFFFFFFFF) == (0, 5)
    assert bytes(svo.device_view()) == view and bytes(svo.info()) == info and same(octree(svo), before)
    assert mv.allocation_state()[:2] == allocs  # the same arrays at the same addresses: no rebuild
    with pytest.raises(mv.MvrtError, match="would leave no voxel"):
        svo.keep_components(K.FACES, 9)
    assert bytes(svo.device_view()) == view and bytes(svo.info()) == info and same(octree(svo), before)
    assert mv.allocation_state()[:2] == allocs


# ---- every flavour, every way a handle comes to its codes ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed():
    return S.sorted_voxels(specks_and_block([(1, 1, 1), (10, 10, 1)]))


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_every_flavour(mv, mixed, flags):
    svo = build(mv, mixed, 32, flags)
    assert flags != 3 or svo.info().flavour == 2  # the tree flavour
    assert_listing(svo, 32)
    for e in ELEMENTS:
        after = assert_keep(mv, mixed, 32, e, min_voxels=2, flags=flags)
        assert after.info().flavour == svo.info().flavour
    svo.set_emission_scale(2.5)
    assert_keep(mv, mixed, 32, K.CUBE, keep_largest=1, flags=flags, svo=svo)


def dumbbell():
    """two 5^3 blocks joined by a bridge one voxel thick: an opening removes the bridge, the blocks stay"""
    g = np.zeros((32, 32, 32), bool)
    g[2:7, 2:7, 2:7] = g[14:19, 2:7, 2:7] = True
    g[7:14, 4, 4] = True
    return np.argwhere(g)


def test_after_an_edit_a_fill_an_opening_and_a_rebuild(mv):
    g = np.zeros((16, 16, 16), bool)
    g[4:11, 4:11, 4:11] = True
    g[5:10, 5:10, 5:10] = False
    svo = build(mv, np.argwhere(g), 16)
    svo.edit_voxels(np.array([(7, 7, 7), (1, 1, 1), (13, 1, 1), (14, 2, 2)], np.uint32), colours(4, 8))  # a voxel inside the cavity and specks outside
    svo.edit_voxels(np.array([(4, 4, 4)], np.uint32), None, np.full(1, REMOVE, np.uint8))
    got = assert_listing(svo, 16)
    assert len(got[K.FACES]["size"]) == 5 and len(got[K.CUBE]["size"]) == 4
    assert svo.fill_enclosed() == 124  # the cavity joins its voxel to the shell
    got = assert_listing(svo, 16)
    assert len(got[K.FACES]["size"]) == 4
    assert_keep(mv, None, 16, K.CUBE, min_voxels=2, svo=svo)
    # an opening that detaches a piece
    bell = build(mv, dumbbell(), 32)
    assert len(assert_listing(bell, 32)[K.CUBE]["size"]) == 1
    assert bell.open(K.CUBE, 1) > 0
    assert assert_listing(bell, 32)[K.CUBE]["size"].tolist() == [125, 125]
    assert_keep(mv, None, 32, K.CUBE, keep_largest=1, svo=bell)
    assert bell.info().numberOfVoxels == 125
    # an upload keeps no codes; after rebuild() it has them
    x0, a0 = svo.read_voxels()
    nodes, attrs, _ = svo.download()
    i = svo.info()
    up = mv.IntersectorOctreeGPU()
    up.upload(nodes, attrs, LOWER, DPS, 16, i.hasEmission, embeddedMask=bool(i.embeddedMask))
    for call in (up.components_device, up.components, up.keep_components):
        with pytest.raises(mv.MvrtError, match="keeps no Morton codes"):
            call()
    up.rebuild()
    assert_listing(up, 16)
    assert_keep(mv, None, 16, K.FACES, keep_largest=1, svo=up)


def test_bunny_at_128(mv):
    tris = bunny_tris()
    v = tris.reshape(-1, 3)
    lo = v.min(0)
    dps = np.float32((v.max(0) - lo).max() / np.float32(128))
    svo = mv.IntersectorOctreeGPU()
    svo.build(v, None, None, None, lo, dps, 128)
    got = assert_listing(svo, 128)
    for e in ELEMENTS:
        print("bunny element", e, "components", len(got[e]["size"]), "five largest", np.sort(got[e]["size"])[::-1][:5].tolist())
    x0, a0 = svo.read_voxels()
    if len(got[K.FACES]["size"]) > 1:
        removed, kept = svo.keep_components(K.FACES, keep_largest=1)
        assert kept == 1 and same(svo.read_voxels(), K.keep(x0, a0, 128, K.FACES, keep_largest=1))


def test_through_the_path_tracers_intersector_with_steps_in_flight(mv):
    """The same two steps around the call and around the edit it stands for: the step issued before finishes first on the old octree, the frame buffer is not
    cleared, and the second step accumulates on it."""
    tris = bunny_tris()
    v = tris.reshape(-1, 3)
    lo = v.min(0)
    res, w, h = 64, 64, 36
    dps = np.float32((v.max(0) - lo).max() / np.float32(res))
    rgba, hw, hh = mv.read_rgbe_file(os.path.join(GOLDEN, "monks_forest_s.hdr"))
    cam = probe_camera(lo, dps, res, focus=9.0, lens_r=0.05)
    base = mv.IntersectorOctreeGPU()
    base.build(v, None, None, None, lo, dps, res)
    x0, a0 = base.read_voxels()
    specks = np.array([(1, 1, 1), (2, 1, 1), (60, 60, 3)], np.uint32)  # debris next to the model
    assert not np.isin(S.morton(specks), S.morton(x0)).any()
    wx, wa = K.keep(np.concatenate([x0, specks]), np.concatenate([a0, colours(3, 3)]), res, K.CUBE, min_voxels=3)
    gone = K.dropped(np.concatenate([x0, specks]), res, K.CUBE, min_voxels=3)
    assert 0 < len(gone) and len(wx) + len(gone) == len(x0) + 3
    frames = []
    for use_call in (True, False):
        pt = mv.PathTracer()
        pt.setup(None)
        pt.resizeFrameBufferIfNeeded(None, w, h)
        pt.loadHDRIPixels(None, rgba, hw, hh, rgba, hw, hh)
        svo = pt.m_intersectorOctreeGPU
        svo.build_voxels(np.concatenate([x0, specks]).astype(np.uint32), np.concatenate([a0, colours(3, 3)]), origin=lo, dps=dps, gridRes=res)
        pt.step(None, cam)
        if use_call:
            assert svo.keep_components(K.CUBE, min_voxels=3)[0] == len(gone)
        else:
            svo.edit_voxels(gone.astype(np.uint32), None, np.full(len(gone), REMOVE, np.uint8))
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
    x0, _ = svo.read_voxels()
    want = K.components(x0, 32, K.CUBE)
    n, nv, big = len(want["size"]), len(x0), int(want["size"].max())
    assert n > 10
    label, size, first, box = mv.DeviceArray(nv, np.uint32), mv.DeviceArray(n, np.uint32), mv.DeviceArray(n, np.uint32), mv.DeviceArray((n, 6), np.uint32)
    assert svo.components_device(K.CUBE) == (n, big)  # the sizing call
    assert svo.components_device(K.CUBE, label) == (n, big) and np.array_equal(label.to_host(), want["label"])  # no per-component array: the capacity is not asked
    assert svo.components_device(K.CUBE, None, n, size) == (n, big) and np.array_equal(size.to_host(), want["size"])
    assert svo.components_device(K.CUBE, None, n, None, first) == (n, big) and np.array_equal(first.to_host(), want["first"])
    assert svo.components_device(K.CUBE, None, n, None, None, box) == (n, big) and np.array_equal(box.to_host(), want["box"])
    lib = mv.lib()
    assert lib.mvrt_svo_components(svo._h, K.CUBE, None, 0, None, None, None, None, None, None) == 0  # even the counts may be NULL
    one = build(mv, [(1, 1, 1), (3, 3, 3)], 4)
    assert lib.mvrt_svo_keep_components(one._h, K.CUBE, 1, 1, None, None, None) == 0 and one.info().numberOfVoxels == 1
    wide, host = filled(mv, (n + 5, 6), np.uint32)  # a larger capacity writes the count's worth
    assert svo.components_device(K.CUBE, None, n + 5, None, None, wide) == (n, big)
    assert np.array_equal(wide.to_host()[:n], want["box"]) and np.array_equal(wide.to_host()[n:], host[n:])
    # one short: the counts are still returned and nothing is written, the labels included
    (label, label_host), (size, size_host), (first, first_host), (box, box_host) = (filled(mv, nv, np.uint32), filled(mv, n, np.uint32), filled(mv, n, np.uint32),
                                                                                   filled(mv, (n, 6), np.uint32))
    nc, nl = C.c_uint64(0), C.c_uint64(0)
    assert lib.mvrt_svo_components(svo._h, K.CUBE, label.ptr, n - 1, size.ptr, first.ptr, box.ptr, C.byref(nc), C.byref(nl), None) != 0
    assert (nc.value, nl.value) == (n, big) and b"componentCapacity %d" % (n - 1) in lib.mvrt_last_error() and b"%d components" % n in lib.mvrt_last_error()
    for dev, host in ((label, label_host), (size, size_host), (first, first_host), (box, box_host)):
        assert np.array_equal(dev.to_host(), host)
    with pytest.raises(mv.MvrtError, match="nothing was written"):
        svo.components_device(K.FACES, label, 0, size)
    assert np.array_equal(label.to_host(), label_host) and np.array_equal(size.to_host(), size_host)


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
        for call in (h.components_device, h.keep_components):
            with pytest.raises(mv.MvrtError, match=text):
                call()
    for call in (svo.components_device, svo.keep_components):
        for e in (-1, 2):
            with pytest.raises(mv.MvrtError, match="unknown element"):
                call(e)
    with pytest.raises(mv.MvrtError, match="minVoxels 0"):
        svo.keep_components(K.CUBE, 0)
    assert mv.allocation_state()[2] == allocs  # on the host, before any GPU work
    assert bytes(svo.info()) == info and same(octree(svo), before)


def test_the_listing_does_not_modify_the_handle(mv, small):
    svo = small
    before, info, held = octree(svo), bytes(svo.info()), mv.allocation_state()[:2]
    assert_listing(svo, 32)
    assert bytes(svo.info()) == info and same(octree(svo), before)
    assert mv.allocation_state()[:2] == held  # the scratch is gone
