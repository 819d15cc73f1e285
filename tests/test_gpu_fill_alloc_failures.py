"""Every device allocation of mvrt_svo_enclosed_cells and mvrt_svo_fill_enclosed is made to fail in turn (mvrt_test_fail_allocation), like
tests/test_gpu_surface_alloc_failures.py does for the surface calls and tests/test_gpu_alloc_failures.py for the edits.  The listing only reads the handle: each
failure names the hook, leaves the octree bit-identical and the caller's arrays untouched, and mvrt_test_allocation_state returns to where it was.  The fill
follows the edit: up to the adoption of the new arrays a failure leaves the old octree whole, from there on an empty handle, and nothing leaks either way."""
import numpy as np
import pytest

import fill_expected as F

pytestmark = pytest.mark.gpu

LOWER, DPS, RES = np.array([-0.3, 0.7, 1.1], np.float32), np.float32(0.013), 32


@pytest.fixture(scope="module")
def mv():
    import massivevoxelraytracing_amd as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def voxels():
    rng = np.random.default_rng(31)
    xyz = np.argwhere(rng.random((RES, RES, RES)) < 0.7).astype(np.uint32)
    return xyz, F.enclosed(xyz, RES)


def build(mv, svo, xyz):
    svo.build_voxels(xyz, None, origin=LOWER, dps=DPS, gridRes=RES)


def filled(mv, shape, dtype):
    host = np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, 0x5A, np.uint8).view(dtype).reshape(shape)
    return mv.DeviceArray.from_host(host), host


def test_each_allocation_of_the_listing_fails_in_turn(mv, voxels):
    xyz, want = voxels
    n = len(want["xyz"])
    assert n > 100
    svo = mv.IntersectorOctreeGPU()
    build(mv, svo, xyz)
    (dx, hx), (dr, hr) = filled(mv, (n, 3), np.uint32), filled(mv, n, np.uint32)
    octree, info, state = svo.download(want_morton=True), bytes(svo.info()), mv.allocation_state()
    assert svo.enclosed_cells_device(n, dx, dr) == (n, want["nRegions"])
    total = mv.allocation_state()[2] - state[2]
    assert total >= 14  # counter, keys, sorted keys, sort storage, parents, offsets, scan storage; pairs twice, sort storage, first cells, ranks, scan storage
    assert mv.allocation_state()[:2] == state[:2]
    for d, h in ((dx, hx), (dr, hr)):  # back to the canary for the sweep
        mv.lib().mvrt_memcpy_h2d(d.ptr, h.ctypes.data, d.nbytes, None)
    for k in range(1, total + 1):
        mv.set_test_fail_allocation(k)
        with pytest.raises(mv.MvrtError, match="mvrt_test_fail_allocation"):
            svo.enclosed_cells_device(n, dx, dr)
        assert mv.lib().mvrt_test_fail_allocation(0) == 0
        assert mv.allocation_state()[:2] == state[:2], k  # nothing leaked
        assert bytes(svo.info()) == info and all(np.array_equal(a, b) for a, b in zip(svo.download(want_morton=True), octree)), k
        assert np.array_equal(dx.to_host(), hx) and np.array_equal(dr.to_host(), hr), k  # the caller's arrays are written last, behind every allocation
    print("listing: allocations failed in turn:", total)
    assert svo.enclosed_cells_device(n, dx, dr) == (n, want["nRegions"])
    assert np.array_equal(dx.to_host(), want["xyz"]) and np.array_equal(dr.to_host(), want["region"])


def test_each_allocation_of_the_fill_fails_in_turn(mv, voxels):
    xyz, want = voxels
    n = len(want["xyz"])
    glow = np.array([9, 8, 7, 255, 6, 0, 0, 255], np.uint8)
    twin = mv.IntersectorOctreeGPU()
    build(mv, twin, xyz)
    twin.edit_voxels(want["xyz"], np.tile(glow, (n, 1)))
    expected = twin.download(want_morton=True)
    base = mv.allocation_state()[:2]
    svo = mv.IntersectorOctreeGPU()
    build(mv, svo, xyz)
    held = tuple(a - b for a, b in zip(mv.allocation_state()[:2], base))
    octree, info = svo.download(want_morton=True), bytes(svo.info())
    before = mv.allocation_state()[2]
    assert svo.fill_enclosed(glow) == n
    total = mv.allocation_state()[2] - before
    assert total >= 20 and all(np.array_equal(a, b) for a, b in zip(svo.download(want_morton=True), expected))
    ends = []
    for k in range(1, total + 1):
        build(mv, svo, xyz)
        assert bytes(svo.info()) == info and tuple(a - b for a, b in zip(mv.allocation_state()[:2], base)) == held
        mv.set_test_fail_allocation(k)
        with pytest.raises(mv.MvrtError, match="mvrt_test_fail_allocation"):
            svo.fill_enclosed(glow)
        assert mv.lib().mvrt_test_fail_allocation(0) == 0
        live = tuple(a - b for a, b in zip(mv.allocation_state()[:2], base))
        if svo.info().numberOfNodes == 0:  # behind the adoption: an empty handle that every reader refuses
            ends.append("empty")
            assert live == (0, 0), k
            with pytest.raises(mv.MvrtError, match="no octree"):
                svo.enclosed_cells_device()
        else:
            ends.append("old")
            assert live == held, k
            assert bytes(svo.info()) == info and all(np.array_equal(a, b) for a, b in zip(svo.download(want_morton=True), octree)), k
    print("fill: allocations failed in turn:", total, "-- old octree kept by the first", ends.count("old"))
    assert ends == sorted(ends, reverse=True) and ends[0] == "old" and ends[-1] == "empty"  # the old octree up to one point of the call, none from there on
    build(mv, svo, xyz)
    assert svo.fill_enclosed(glow) == n
    assert all(np.array_equal(a, b) for a, b in zip(svo.download(want_morton=True), expected))
