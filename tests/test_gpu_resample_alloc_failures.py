"""Every device allocation of the two resampling calls is made to fail in turn (mvrt_test_fail_allocation), like tests/test_gpu_combine_alloc_failures.py does for
the two-set calls.  The listing only reads the handle: each failure names the hook, leaves the octree bit-identical and the caller's arrays untouched, and
mvrt_test_allocation_state returns to where it was.  The build follows the voxel-list build, as mvrt.h says: up to the adoption of the new arrays a failure leaves
dst bit-identical to what it was, from there on (the derived tables, made after the old octree is released) an empty handle; src stays bit-identical and nothing
leaks either way."""
import numpy as np
import pytest

import resample_expected as E

pytestmark = pytest.mark.gpu

LOWER, DPS, RES = np.array([-0.3, 0.7, 1.1], np.float32), np.float32(0.013), 32
TURN = E.rotation((1, 2, 3), 30.0)


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


def build(svo, v, res=RES):
    svo.build_voxels(v[0], v[1], origin=LOWER, dps=DPS, gridRes=res)


def filled(mv, shape, dtype):
    host = np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, 0x5A, np.uint8).view(dtype).reshape(shape)
    return mv.DeviceArray.from_host(host), host


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("rd", [32, 64])
def test_each_allocation_of_the_listing_fails_in_turn(mv, rd):
    src = mv.IntersectorOctreeGPU()
    build(src, voxels(31))
    mt = E.about_centre(TURN * (RES / rd), RES, rd)
    xf = mv.CellTransform.make(*mt)
    want = E.dense(*src.read_voxels(), RES, mt[0], mt[1], rd)
    n = len(want["xyz"])
    assert n > 1000
    arrays = (filled(mv, (n, 3), np.uint32), filled(mv, (n, 8), np.uint8), filled(mv, n, np.uint32))
    whole = (src.download(want_morton=True), bytes(src.info()))
    call = lambda: src.resample_voxels_device(xf, rd, n, arrays[0][0], arrays[1][0], arrays[2][0])
    state = mv.allocation_state()
    assert call() == n
    total = mv.allocation_state()[2] - state[2]
    levels = rd.bit_length() - 1
    assert total >= 1 + 3 * levels + (levels - 1) and mv.allocation_state()[:2] == state[:2]  # the root; masks, offsets and scan storage per level; a frontier per level but the last
    for d, h in arrays:  # back to the canary for the sweep
        mv.lib().mvrt_memcpy_h2d(d.ptr, h.ctypes.data, d.nbytes, None)
    for k in range(1, total + 1):
        mv.set_test_fail_allocation(k)
        with pytest.raises(mv.MvrtError, match="mvrt_test_fail_allocation"):
            call()
        assert mv.lib().mvrt_test_fail_allocation(0) == 0
        assert mv.allocation_state()[:2] == state[:2], k  # nothing leaked
        assert bytes(src.info()) == whole[1] and same(src.download(want_morton=True), whole[0]), k
        assert all(np.array_equal(d.to_host(), h) for d, h in arrays), k  # the caller's arrays are written last, behind every allocation
    print("listing, Rd", rd, ": allocations failed in turn:", total)
    assert call() == n
    assert all(np.array_equal(d.to_host(), want[key]) for (d, _), key in zip(arrays, ("xyz", "attribs", "source")))


@pytest.mark.parametrize("in_place", [False, True])
def test_each_allocation_of_the_build_fails_in_turn(mv, in_place):
    mt = E.about_centre(TURN, RES, RES)
    xf = mv.CellTransform.make(*mt)
    base = mv.allocation_state()[:2]
    src, dst = mv.IntersectorOctreeGPU(), mv.IntersectorOctreeGPU()
    v_src, v_dst = voxels(31), voxels(35)
    build(src, v_src)
    src_whole = (src.download(want_morton=True), bytes(src.info()))
    held_src = tuple(x - y for x, y in zip(mv.allocation_state()[:2], base))
    if in_place:
        dst, v_dst, held_src = src, v_src, (0, 0)
    else:
        build(dst, v_dst)
    held = tuple(x - y for x, y in zip(mv.allocation_state()[:2], base))
    octree, info = dst.download(want_morton=True), bytes(dst.info())
    want = E.dense(*src.read_voxels(), RES, mt[0], mt[1], RES)
    before = mv.allocation_state()[2]
    src.resample(xf, dst)
    total = mv.allocation_state()[2] - before
    expected = dst.download(want_morton=True)
    assert total >= 20 and same(dst.read_voxels(), (want["xyz"], want["attribs"]))
    ends = []
    for k in range(1, total + 1):
        build(dst, v_dst)
        assert bytes(dst.info()) == info and tuple(x - y for x, y in zip(mv.allocation_state()[:2], base)) == held
        mv.set_test_fail_allocation(k)
        with pytest.raises(mv.MvrtError, match="mvrt_test_fail_allocation"):
            src.resample(xf, dst)
        assert mv.lib().mvrt_test_fail_allocation(0) == 0
        live = tuple(x - y for x, y in zip(mv.allocation_state()[:2], base))
        if not in_place:
            assert bytes(src.info()) == src_whole[1] and same(src.download(want_morton=True), src_whole[0]), k
        if dst.info().numberOfNodes == 0:  # behind the adoption: an empty handle that every reader refuses
            ends.append("empty")
            assert live == held_src, k
            with pytest.raises(mv.MvrtError, match="no octree"):
                dst.resample_voxels_device(xf, RES)
        else:
            ends.append("old")
            assert live == held, k
            assert bytes(dst.info()) == info and same(dst.download(want_morton=True), octree), k
    print("resample, in place", in_place, ": allocations failed in turn:", total, "-- old octree kept by the first", ends.count("old"))
    assert ends == sorted(ends, reverse=True) and ends[0] == "old" and ends.count("old") >= 20  # every allocation of the refinement and of the levels keeps dst whole
    build(dst, v_dst)
    src.resample(xf, dst)
    assert same(dst.download(want_morton=True), expected)
