"""Every device allocation of mvrt_svo_enclosed_nearest and mvrt_svo_fill_enclosed_nearest is made to fail in turn (mvrt_test_fail_allocation), like
tests/test_gpu_fill_alloc_failures.py does for the plain fill, on the 32^3 block among noise of tests/test_gpu_ball_alloc_failures.py with the block hollowed out.
The listing only reads the handle: each failure names the hook, leaves the octree bit-identical and the caller's arrays untouched, and
mvrt_test_allocation_state returns to where it was.  The fill follows the edit: up to the adoption of the new arrays a failure leaves the old octree whole, from
there on an empty handle, and nothing leaks either way."""
import numpy as np
import pytest

import nearest_expected as N

pytestmark = pytest.mark.gpu

LOWER, DPS, RES = np.array([-0.3, 0.7, 1.1], np.float32), np.float32(0.013), 32
KEYS = ("xyz", "region", "dist2", "nearest", "attribs")


@pytest.fixture(scope="module")
def mv():
    import massivevoxelraytracing_amd as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def voxels():
    rng = np.random.default_rng(31)
    solid = np.zeros((RES, RES, RES), bool)
    solid[8:20, 8:20, 8:20] = True
    solid |= rng.random((RES, RES, RES)) < 0.03
    solid[9:19, 9:19, 9:19] &= rng.random((10, 10, 10)) < 0.03  # hollowed: a cavity of 10^3 with the noise left in it
    xyz = np.argwhere(solid).astype(np.uint32)
    at = rng.integers(0, 256, (len(xyz), 8), dtype=np.uint8)
    return xyz, at, N.enclosed_nearest(xyz, at, RES)


def build(svo, xyz, at):
    svo.build_voxels(xyz, at, origin=LOWER, dps=DPS, gridRes=RES)


def filled(mv, shape, dtype):
    host = np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, 0x5A, np.uint8).view(dtype).reshape(shape)
    return mv.DeviceArray.from_host(host), host


def test_each_allocation_of_the_listing_fails_in_turn(mv, voxels):
    xyz, at, want = voxels
    n = len(want["xyz"])
    assert n > 900
    svo = mv.IntersectorOctreeGPU()
    build(svo, xyz, at)
    shapes = {"xyz": ((n, 3), np.uint32), "region": (n, np.uint32), "dist2": (n, np.uint32), "nearest": (n, np.uint32), "attribs": ((n, 8), np.uint8)}
    arrays = {k: filled(mv, *shapes[k]) for k in KEYS}
    dev = {k: arrays[k][0] for k in KEYS}
    octree, info, state = svo.download(want_morton=True), bytes(svo.info()), mv.allocation_state()
    assert svo.enclosed_nearest_device(n, **dev) == (n, want["nRegions"])
    total = mv.allocation_state()[2] - state[2]
    assert total >= 40  # the classification's 7, the counters and the x pass's 4, per pass the sort's 3 and 8 more, the last sort's 3, roots, first cells, ranks, scan storage
    assert mv.allocation_state()[:2] == state[:2]
    for d, h in arrays.values():  # back to the canary for the sweep
        mv.lib().mvrt_memcpy_h2d(d.ptr, h.ctypes.data, d.nbytes, None)
    for k in range(1, total + 1):
        mv.set_test_fail_allocation(k)
        with pytest.raises(mv.MvrtError, match="mvrt_test_fail_allocation"):
            svo.enclosed_nearest_device(n, **dev)
        assert mv.lib().mvrt_test_fail_allocation(0) == 0
        assert mv.allocation_state()[:2] == state[:2], k  # nothing leaked
        assert bytes(svo.info()) == info and all(np.array_equal(a, b) for a, b in zip(svo.download(want_morton=True), octree)), k
        assert all(np.array_equal(d.to_host(), h) for d, h in arrays.values()), k  # the caller's arrays are written last, behind every allocation
    print("listing: allocations failed in turn:", total)
    assert svo.enclosed_nearest_device(n, **dev) == (n, want["nRegions"])
    assert all(np.array_equal(dev[k].to_host(), want[k]) for k in KEYS)


def test_each_allocation_of_the_fill_fails_in_turn(mv, voxels):
    xyz, at, want = voxels
    n = len(want["xyz"])
    twin = mv.IntersectorOctreeGPU()
    build(twin, xyz, at)
    twin.edit_voxels(want["xyz"], want["attribs"])
    expected = twin.download(want_morton=True)
    base = mv.allocation_state()[:2]
    svo = mv.IntersectorOctreeGPU()
    build(svo, xyz, at)
    held = tuple(a - b for a, b in zip(mv.allocation_state()[:2], base))
    octree, info = svo.download(want_morton=True), bytes(svo.info())
    before = mv.allocation_state()[2]
    assert svo.fill_enclosed_nearest() == n
    total = mv.allocation_state()[2] - before
    assert total >= 40 and all(np.array_equal(a, b) for a, b in zip(svo.download(want_morton=True), expected))
    ends = []
    for k in range(1, total + 1):
        build(svo, xyz, at)
        assert bytes(svo.info()) == info and tuple(a - b for a, b in zip(mv.allocation_state()[:2], base)) == held
        mv.set_test_fail_allocation(k)
        with pytest.raises(mv.MvrtError, match="mvrt_test_fail_allocation"):
            svo.fill_enclosed_nearest()
        assert mv.lib().mvrt_test_fail_allocation(0) == 0
        live = tuple(a - b for a, b in zip(mv.allocation_state()[:2], base))
        if svo.info().numberOfNodes == 0:  # behind the adoption: an empty handle that every reader refuses
            ends.append("empty")
            assert live == (0, 0), k
            with pytest.raises(mv.MvrtError, match="no octree"):
                svo.enclosed_nearest_device()
        else:
            ends.append("old")
            assert live == held, k
            assert bytes(svo.info()) == info and all(np.array_equal(a, b) for a, b in zip(svo.download(want_morton=True), octree)), k
    print("fill: allocations failed in turn:", total, "-- old octree kept by the first", ends.count("old"))
    assert ends == sorted(ends, reverse=True) and ends[0] == "old" and ends[-1] == "empty"  # the old octree up to one point of the call, none from there on
    build(svo, xyz, at)
    assert svo.fill_enclosed_nearest() == n
    assert all(np.array_equal(a, b) for a, b in zip(svo.download(want_morton=True), expected))
