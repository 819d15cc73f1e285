"""Every device allocation of the two component calls is made to fail in turn (mvrt_test_fail_allocation), like tests/test_gpu_morph_alloc_failures.py does for the
morphology.  The listing only reads the handle: each failure names the hook, leaves the octree bit-identical and the caller's arrays untouched, and
mvrt_test_allocation_state returns to where it was.  The in-place call follows the edit: up to the adoption of the new arrays a failure leaves the old octree
whole, from there on an empty handle, and nothing leaks either way."""
import numpy as np
import pytest

import components_expected as K

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


@pytest.mark.parametrize("element", [K.FACES, K.CUBE])
def test_each_allocation_of_the_listing_fails_in_turn(mv, voxels, element):
    svo = mv.IntersectorOctreeGPU()
    build(svo, voxels)
    x0, _ = svo.read_voxels()
    want = K.components(x0, RES, element)
    n, big = len(want["size"]), int(want["size"].max())
    assert n > 100
    (dl, hl), (ds, hs), (df, hf), (db, hb) = filled(mv, len(x0), np.uint32), filled(mv, n, np.uint32), filled(mv, n, np.uint32), filled(mv, (n, 6), np.uint32)
    arrays = ((dl, hl), (ds, hs), (df, hf), (db, hb))
    octree, info = svo.download(want_morton=True), bytes(svo.info())
    call = lambda: svo.components_device(element, dl, n, ds, df, db)
    state = mv.allocation_state()
    assert call() == (n, big)
    total = mv.allocation_state()[2] - state[2]
    assert total >= 6 and mv.allocation_state()[:2] == state[:2]  # parents, ranks, scan storage, sizes, boxes, the largest
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
    assert call() == (n, big)
    assert np.array_equal(dl.to_host(), want["label"]) and np.array_equal(ds.to_host(), want["size"])
    assert np.array_equal(df.to_host(), want["first"]) and np.array_equal(db.to_host(), want["box"])


@pytest.mark.parametrize("element,min_voxels,keep_largest", [(K.FACES, 2, 0), (K.CUBE, 1, 1)])
def test_each_allocation_of_the_in_place_call_fails_in_turn(mv, voxels, element, min_voxels, keep_largest):
    base = mv.allocation_state()[:2]
    svo = mv.IntersectorOctreeGPU()
    build(svo, voxels)
    held = tuple(a - b for a, b in zip(mv.allocation_state()[:2], base))
    octree, info = svo.download(want_morton=True), bytes(svo.info())
    x0, a0 = svo.read_voxels()
    wx, wa = K.keep(x0, a0, RES, element, min_voxels, keep_largest)
    before = mv.allocation_state()[2]
    assert svo.keep_components(element, min_voxels, keep_largest)[0] == len(x0) - len(wx) > 0
    total = mv.allocation_state()[2] - before
    expected = svo.download(want_morton=True)
    assert total >= 10 and same(svo.read_voxels(), (wx, wa))
    ends = []
    for k in range(1, total + 1):
        build(svo, voxels)
        assert bytes(svo.info()) == info and tuple(a - b for a, b in zip(mv.allocation_state()[:2], base)) == held
        mv.set_test_fail_allocation(k)
        with pytest.raises(mv.MvrtError, match="mvrt_test_fail_allocation"):
            svo.keep_components(element, min_voxels, keep_largest)
        assert mv.lib().mvrt_test_fail_allocation(0) == 0
        live = tuple(a - b for a, b in zip(mv.allocation_state()[:2], base))
        if svo.info().numberOfNodes == 0:  # behind the adoption: an empty handle that every reader refuses
            ends.append("empty")
            assert live == (0, 0), k
            with pytest.raises(mv.MvrtError, match="no octree"):
                svo.components_device()
        else:
            ends.append("old")
            assert live == held, k
            assert bytes(svo.info()) == info and same(svo.download(want_morton=True), octree), k
    print("keep_components: allocations failed in turn:", total, "-- old octree kept by the first", ends.count("old"))
    assert ends == sorted(ends, reverse=True) and ends[0] == "old" and ends[-1] == "empty"  # the old octree up to one point of the call, none from there on
    build(svo, voxels)
    svo.keep_components(element, min_voxels, keep_largest)
    assert same(svo.download(want_morton=True), expected)
