"""Every device allocation of mvrt_svo_coarse_voxels and mvrt_svo_coarsen is made to fail in turn (mvrt_test_fail_allocation), like
tests/test_gpu_fill_alloc_failures.py does for the fill.  The listing only reads the handle: each failure names the hook, leaves the octree bit-identical and the
caller's arrays untouched, and mvrt_test_allocation_state returns to where it was.  The build follows the voxel-list build: up to the adoption of the new arrays a
failure leaves the destination as it was, from there on empty; the source, where it is another handle, stays whole; nothing leaks either way."""
import numpy as np
import pytest

import coarsen_expected as X

pytestmark = pytest.mark.gpu

LOWER, DPS, RES = np.array([-0.3, 0.7, 1.1], np.float32), np.float32(0.013), 32


@pytest.fixture(scope="module")
def mv():
    import massivevoxelraytracing_amd as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def voxels():
    rng = np.random.default_rng(51)
    xyz = np.argwhere(rng.random((RES, RES, RES)) < 0.2).astype(np.uint32)
    return xyz, rng.integers(0, 256, size=(len(xyz), 8), dtype=np.uint8)


def build(svo, xyz, attribs, res=RES):
    svo.build_voxels(xyz, attribs, origin=LOWER, dps=DPS, gridRes=res)


def filled(mv, shape, dtype):
    host = np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, 0x5A, np.uint8).view(dtype).reshape(shape)
    return mv.DeviceArray.from_host(host), host


@pytest.mark.parametrize("min_count", [1, 2])
def test_each_allocation_of_the_listing_fails_in_turn(mv, voxels, min_count):
    xyz, attribs = voxels
    want = X.coarse(xyz, attribs, 1, min_count)
    n = len(want["xyz"])
    assert n > 1000
    svo = mv.IntersectorOctreeGPU()
    build(svo, xyz, attribs)
    arrays = [filled(mv, (n, 3), np.uint32), filled(mv, (n, 8), np.uint8), filled(mv, n, np.uint32)]
    octree, info, state = svo.download(want_morton=True), bytes(svo.info()), mv.allocation_state()
    args = (1, min_count, n) + tuple(d for d, _ in arrays)
    assert svo.coarse_voxels_device(*args) == n
    total = mv.allocation_state()[2] - state[2]
    assert total >= (5 if min_count == 1 else 7)  # ranks, scan storage, sums, counts, codes; with a minCount also the places of the kept cells and their scan storage
    assert mv.allocation_state()[:2] == state[:2]
    for d, h in arrays:  # back to the canary for the sweep
        mv.lib().mvrt_memcpy_h2d(d.ptr, h.ctypes.data, d.nbytes, None)
    for k in range(1, total + 1):
        mv.set_test_fail_allocation(k)
        with pytest.raises(mv.MvrtError, match="mvrt_test_fail_allocation"):
            svo.coarse_voxels_device(*args)
        assert mv.lib().mvrt_test_fail_allocation(0) == 0
        assert mv.allocation_state()[:2] == state[:2], k  # nothing leaked
        assert bytes(svo.info()) == info and all(np.array_equal(a, b) for a, b in zip(svo.download(want_morton=True), octree)), k
        assert all(np.array_equal(d.to_host(), h) for d, h in arrays), k  # the caller's arrays are written last, behind every allocation
    print("listing, minCount", min_count, ": allocations failed in turn:", total)
    assert svo.coarse_voxels_device(*args) == n
    assert all(np.array_equal(d.to_host(), want[f]) for (d, _), f in zip(arrays, ("xyz", "attribs", "count")))


@pytest.mark.parametrize("in_place", [False, True])
def test_each_allocation_of_the_build_fails_in_turn(mv, voxels, in_place):
    xyz, attribs = voxels
    want = X.coarse(xyz, attribs, 1, 2)
    twin = mv.IntersectorOctreeGPU()
    twin.build_voxels(want["xyz"], want["attribs"], origin=LOWER, dps=np.float32(DPS * np.float32(2)), gridRes=RES // 2)
    expected = twin.download(want_morton=True)
    old_xyz = np.argwhere(np.ones((4, 4, 4), bool)).astype(np.uint32)  # what the destination holds before, where it is another handle
    base = mv.allocation_state()[:2]
    src, other = mv.IntersectorOctreeGPU(), mv.IntersectorOctreeGPU()
    dst = src if in_place else other

    def reset():
        build(src, xyz, attribs)
        source_alone = tuple(a - b for a, b in zip(mv.allocation_state()[:2], base)) if in_place or other.info().numberOfNodes == 0 else None
        if not in_place:
            build(other, old_xyz, None, 4)
        return source_alone

    held_by_source = reset()  # (the destination is still empty here: what the source alone holds)
    held = tuple(a - b for a, b in zip(mv.allocation_state()[:2], base))
    source, source_info = src.download(want_morton=True), bytes(src.info())
    octree, info = dst.download(want_morton=True), bytes(dst.info())
    before = mv.allocation_state()[2]
    src.coarsen(1, 2, 0, dst)
    total = mv.allocation_state()[2] - before
    assert total >= 15 and all(np.array_equal(a, b) for a, b in zip(dst.download(want_morton=True), expected))
    ends = []
    for k in range(1, total + 1):
        reset()
        assert bytes(dst.info()) == info and tuple(a - b for a, b in zip(mv.allocation_state()[:2], base)) == held
        mv.set_test_fail_allocation(k)
        with pytest.raises(mv.MvrtError, match="mvrt_test_fail_allocation"):
            src.coarsen(1, 2, 0, dst)
        assert mv.lib().mvrt_test_fail_allocation(0) == 0
        live = tuple(a - b for a, b in zip(mv.allocation_state()[:2], base))
        if dst.info().numberOfNodes == 0:  # behind the adoption: an empty handle that every reader refuses
            ends.append("empty")
            assert live == ((0, 0) if in_place else held_by_source), k
            with pytest.raises(mv.MvrtError, match="no octree"):
                dst.coarse_voxels_device(1)
        else:
            ends.append("old")
            assert live == held, k
            assert bytes(dst.info()) == info and all(np.array_equal(a, b) for a, b in zip(dst.download(want_morton=True), octree)), k
        if not in_place:  # the source stays whole throughout
            assert bytes(src.info()) == source_info and all(np.array_equal(a, b) for a, b in zip(src.download(want_morton=True), source)), k
    print("coarsen, in place" if in_place else "coarsen", ": allocations failed in turn:", total, "-- old octree kept by the first", ends.count("old"))
    assert ends == sorted(ends, reverse=True) and ends[0] == "old" and ends[-1] == "empty"  # the old octree up to one point of the call, none from there on
    reset()
    src.coarsen(1, 2, 0, dst)
    assert all(np.array_equal(a, b) for a, b in zip(dst.download(want_morton=True), expected))
