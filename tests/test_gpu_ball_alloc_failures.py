"""Every device allocation of the six round-offset calls is made to fail in turn (mvrt_test_fail_allocation), like tests/test_gpu_morph_alloc_failures.py does for
the morphology, on the same 32^3 block among noise, at radius2 = 5.  The listings only read the handle: each failure names the hook, leaves the octree
bit-identical and the caller's arrays untouched, and mvrt_test_allocation_state returns to where it was.  The in-place calls follow the edit: up to the adoption
of the new arrays a failure leaves the old octree whole, from there on an empty handle, and nothing leaks either way."""
import numpy as np
import pytest

import ball_expected as B

pytestmark = pytest.mark.gpu

LOWER, DPS, RES, RHO = np.array([-0.3, 0.7, 1.1], np.float32), np.float32(0.013), 32, 5


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
    xyz = np.argwhere(solid).astype(np.uint32)
    return xyz, rng.integers(0, 256, (len(xyz), 8), dtype=np.uint8)


def build(svo, voxels):
    svo.build_voxels(voxels[0], voxels[1], origin=LOWER, dps=DPS, gridRes=RES)


def filled(mv, shape, dtype):
    host = np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, 0x5A, np.uint8).view(dtype).reshape(shape)
    return mv.DeviceArray.from_host(host), host


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_each_allocation_of_the_listings_fails_in_turn(mv, voxels):
    svo = mv.IntersectorOctreeGPU()
    build(svo, voxels)
    x0, a0 = svo.read_voxels()
    want = B.distance_cells(x0, a0, RES, RHO)
    gone = B.depth_voxels(x0, RES, RHO)
    n, m = len(want["xyz"]), len(gone["vIndex"])
    assert n > 100 and m > 100
    (dx, hx), (dd, hd), (dn, hn), (da, ha) = filled(mv, (n, 3), np.uint32), filled(mv, n, np.uint32), filled(mv, n, np.uint32), filled(mv, (n, 8), np.uint8)
    (dv, hv), (dp, hp) = filled(mv, m, np.uint32), filled(mv, m, np.uint32)
    octree, info = svo.download(want_morton=True), bytes(svo.info())
    # seed flags, offsets, scan storage, seeds twice, then per pass offsets, scan storage, records three times, sorted twice, sort storage, ranks, ...
    calls = ((lambda: svo.distance_cells_device(RHO, n, dx, dd, dn, da), n, 30, ((dx, hx), (dd, hd), (dn, hn), (da, ha))),
             (lambda: svo.depth_voxels_device(RHO, m, dv, dp), m, 30, ((dv, hv), (dp, hp))))
    for call, count, least, arrays in calls:
        state = mv.allocation_state()
        assert call() == count
        total = mv.allocation_state()[2] - state[2]
        assert total >= least and mv.allocation_state()[:2] == state[:2]
        for d, h in arrays:  # back to the canary for the sweep
            mv.lib().mvrt_memcpy_h2d(d.ptr, h.ctypes.data, d.nbytes, None)
        for k in range(1, total + 1):
            mv.set_test_fail_allocation(k)
            with pytest.raises(mv.MvrtError, match="mvrt_test_fail_allocation"):
                call()
            assert mv.lib().mvrt_test_fail_allocation(0) == 0
            assert mv.allocation_state()[:2] == state[:2], k  # nothing leaked
            assert bytes(svo.info()) == info and same(svo.download(want_morton=True), octree), k
            assert all(np.array_equal(d.to_host(), h) for d, h in arrays), k  # the caller's arrays are written last, behind every allocation
        print("listing: allocations failed in turn:", total)
        assert call() == count
    assert np.array_equal(dx.to_host(), want["xyz"]) and np.array_equal(dd.to_host(), want["dist2"]) and np.array_equal(dn.to_host(), want["nearest"])
    assert np.array_equal(da.to_host(), want["attribs"]) and np.array_equal(dv.to_host(), gone["vIndex"]) and np.array_equal(dp.to_host(), gone["depth2"])


@pytest.mark.parametrize("op", ["dilate", "erode", "close", "open"])
def test_each_allocation_of_an_in_place_call_fails_in_turn(mv, voxels, op):
    base = mv.allocation_state()[:2]
    svo = mv.IntersectorOctreeGPU()
    build(svo, voxels)
    held = tuple(a - b for a, b in zip(mv.allocation_state()[:2], base))
    octree, info = svo.download(want_morton=True), bytes(svo.info())
    x0, a0 = svo.read_voxels()
    wx, wa = B.ball(op, x0, a0, RES, RHO)
    call = getattr(svo, op + "_ball")
    before = mv.allocation_state()[2]
    assert call(RHO) == abs(len(wx) - len(x0)) > 0
    total = mv.allocation_state()[2] - before
    expected = svo.download(want_morton=True)
    assert total >= 30 and same(svo.read_voxels(), (wx, wa))
    ends = []
    for k in range(1, total + 1):
        build(svo, voxels)
        assert bytes(svo.info()) == info and tuple(a - b for a, b in zip(mv.allocation_state()[:2], base)) == held
        mv.set_test_fail_allocation(k)
        with pytest.raises(mv.MvrtError, match="mvrt_test_fail_allocation"):
            call(RHO)
        assert mv.lib().mvrt_test_fail_allocation(0) == 0
        live = tuple(a - b for a, b in zip(mv.allocation_state()[:2], base))
        if svo.info().numberOfNodes == 0:  # behind the adoption: an empty handle that every reader refuses
            ends.append("empty")
            assert live == (0, 0), k
            with pytest.raises(mv.MvrtError, match="no octree"):
                svo.distance_cells_device()
        else:
            ends.append("old")
            assert live == held, k
            assert bytes(svo.info()) == info and same(svo.download(want_morton=True), octree), k
    print(op, "allocations failed in turn:", total, "-- old octree kept by the first", ends.count("old"))
    assert ends == sorted(ends, reverse=True) and ends[0] == "old" and ends[-1] == "empty"  # the old octree up to one point of the call, none from there on
    build(svo, voxels)
    call(RHO)
    assert same(svo.download(want_morton=True), expected)
