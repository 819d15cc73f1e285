"""Every device allocation of the two combine calls is made to fail in turn (mvrt_test_fail_allocation), like tests/test_gpu_components_alloc_failures.py does for
the components, for a zero offset (b's codes as they are) and a non-zero one (translate, compact, sort).  The listing only reads the handles: each failure names
the hook, leaves both octrees bit-identical and the caller's arrays untouched, and mvrt_test_allocation_state returns to where it was.  The in-place call follows
the edit: up to the adoption of the new arrays a failure leaves the old octree whole, from there on an empty handle; b stays whole and nothing leaks either way."""
import numpy as np
import pytest

import combine_expected as E

pytestmark = pytest.mark.gpu

LOWER, DPS, RES = np.array([-0.3, 0.7, 1.1], np.float32), np.float32(0.013), 32
OFFSETS = [None, (3, -2, 1)]


@pytest.fixture(scope="module")
def mv():
    import massivevoxelraytracing_amd as m
    m.lib()
    return m


def voxels(seed):
    rng = np.random.default_rng(seed)
    solid = np.zeros((RES, RES, RES), bool)
    solid[8:20, 8:20, 8:20] = True
    solid |= rng.random((RES, RES, RES)) < 0.03
    xyz = np.argwhere(solid).astype(np.uint32)
    return xyz, rng.integers(0, 256, (len(xyz), 8), dtype=np.uint8)


def build(svo, v):
    svo.build_voxels(v[0], v[1], origin=LOWER, dps=DPS, gridRes=RES)


def filled(mv, shape, dtype):
    host = np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, 0x5A, np.uint8).view(dtype).reshape(shape)
    return mv.DeviceArray.from_host(host), host


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("offset", OFFSETS)
def test_each_allocation_of_the_listing_fails_in_turn(mv, offset):
    a, b = mv.IntersectorOctreeGPU(), mv.IntersectorOctreeGPU()
    build(a, voxels(31))
    build(b, voxels(32))
    (xa, aa), (xb, ab) = a.read_voxels(), b.read_voxels()
    want = E.combine(xa, aa, xb, ab, RES, E.XOR, offset, E.ATTRIB_B)
    n, counts = len(want["xyz"]), (len(want["xyz"]), want["overlap"], want["clipped"])
    assert n > 1000 and want["overlap"] > 500
    arrays = (filled(mv, (n, 3), np.uint32), filled(mv, (n, 8), np.uint8), filled(mv, n, np.uint8))
    whole = [(h.download(want_morton=True), bytes(h.info())) for h in (a, b)]
    call = lambda: a.combine_voxels_device(b, E.XOR, offset, E.ATTRIB_B, n, arrays[0][0], arrays[1][0], arrays[2][0])
    state = mv.allocation_state()
    assert call() == counts
    total = mv.allocation_state()[2] - state[2]
    assert total >= (8 if offset is None else 14) and mv.allocation_state()[:2] == state[:2]  # partner, state, offsets and scan storage per list; + keys, scan, compaction, sort
    for d, h in arrays:  # back to the canary for the sweep
        mv.lib().mvrt_memcpy_h2d(d.ptr, h.ctypes.data, d.nbytes, None)
    for k in range(1, total + 1):
        mv.set_test_fail_allocation(k)
        with pytest.raises(mv.MvrtError, match="mvrt_test_fail_allocation"):
            call()
        assert mv.lib().mvrt_test_fail_allocation(0) == 0
        assert mv.allocation_state()[:2] == state[:2], k  # nothing leaked
        for h, (octree, info) in zip((a, b), whole):
            assert bytes(h.info()) == info and same(h.download(want_morton=True), octree), k
        assert all(np.array_equal(d.to_host(), h) for d, h in arrays), k  # the caller's arrays are written last, behind every allocation
    print("listing, offset", offset, ": allocations failed in turn:", total)
    assert call() == counts
    assert all(np.array_equal(d.to_host(), want[key]) for (d, _), key in zip(arrays, ("xyz", "attribs", "source")))


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("op,flags", [(E.UNION, E.ATTRIB_B), (E.DIFFERENCE, 0)])
def test_each_allocation_of_the_in_place_call_fails_in_turn(mv, offset, op, flags):
    b = mv.IntersectorOctreeGPU()
    build(b, voxels(32))
    b_whole = (b.download(want_morton=True), bytes(b.info()))
    base = mv.allocation_state()[:2]
    a = mv.IntersectorOctreeGPU()
    va = voxels(31)
    build(a, va)
    held = tuple(x - y for x, y in zip(mv.allocation_state()[:2], base))
    octree, info = a.download(want_morton=True), bytes(a.info())
    (xa, aa), (xb, ab) = a.read_voxels(), b.read_voxels()
    want = E.combine(xa, aa, xb, ab, RES, op, offset, flags)
    before = mv.allocation_state()[2]
    added, removed, clipped = a.combine(b, op, offset, flags)
    total = mv.allocation_state()[2] - before
    expected = a.download(want_morton=True)
    assert added + removed > 0 and clipped == want["clipped"] and total >= 12 and same(a.read_voxels(), (want["xyz"], want["attribs"]))
    ends = []
    for k in range(1, total + 1):
        build(a, va)
        assert bytes(a.info()) == info and tuple(x - y for x, y in zip(mv.allocation_state()[:2], base)) == held
        mv.set_test_fail_allocation(k)
        with pytest.raises(mv.MvrtError, match="mvrt_test_fail_allocation"):
            a.combine(b, op, offset, flags)
        assert mv.lib().mvrt_test_fail_allocation(0) == 0
        live = tuple(x - y for x, y in zip(mv.allocation_state()[:2], base))
        assert bytes(b.info()) == b_whole[1] and same(b.download(want_morton=True), b_whole[0]), k
        if a.info().numberOfNodes == 0:  # behind the adoption: an empty handle that every reader refuses
            ends.append("empty")
            assert live == (0, 0), k
            with pytest.raises(mv.MvrtError, match="no octree"):
                a.combine_voxels_device(b, op)
        else:
            ends.append("old")
            assert live == held, k
            assert bytes(a.info()) == info and same(a.download(want_morton=True), octree), k
    print("combine op", op, "offset", offset, ": allocations failed in turn:", total, "-- old octree kept by the first", ends.count("old"))
    assert ends == sorted(ends, reverse=True) and ends[0] == "old" and ends[-1] == "empty"  # the old octree up to one point of the call, none from there on
    build(a, va)
    a.combine(b, op, offset, flags)
    assert same(a.download(want_morton=True), expected)


def test_each_allocation_of_a_recolouring_fails_in_turn(mv):
    """the attribute-only call writes in place, behind its last allocation: every failure leaves the old bytes"""
    va = voxels(31)
    a, b = mv.IntersectorOctreeGPU(), mv.IntersectorOctreeGPU()
    build(a, va)
    build(b, (va[0], np.random.default_rng(33).integers(0, 256, (len(va[0]), 8), dtype=np.uint8)))  # the same cells in other colours
    octree, info, state = a.download(want_morton=True), bytes(a.info()), mv.allocation_state()
    before = state[2]
    assert a.combine(b, E.INTERSECTION, None, E.ATTRIB_B) == (0, 0, 0) and same(a.read_voxels(), b.read_voxels())
    total = mv.allocation_state()[2] - before
    assert total >= 8 and mv.allocation_state()[:2] == state[:2]
    for k in range(1, total + 1):
        build(a, va)
        mv.set_test_fail_allocation(k)
        with pytest.raises(mv.MvrtError, match="mvrt_test_fail_allocation"):
            a.combine(b, E.INTERSECTION, None, E.ATTRIB_B)
        assert mv.lib().mvrt_test_fail_allocation(0) == 0
        assert mv.allocation_state()[:2] == state[:2], k
        assert bytes(a.info()) == info and same(a.download(want_morton=True), octree), k
