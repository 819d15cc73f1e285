"""Every device allocation of mvrt_svo_surface_exterior_masks and of mvrt_svo_surface_quads_masked is made to fail in turn (mvrt_test_fail_allocation), like
tests/test_gpu_fill_alloc_failures.py does for the listing.  Both calls only read the handle: each failure names the hook, leaves the octree bit-identical and
the caller's arrays untouched, mvrt_test_allocation_state returns to where it was, and the call succeeds again afterwards."""
import numpy as np
import pytest

import exterior_expected as E
import surface_expected as S

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
    return xyz, E.exterior(xyz, RES)


def filled(mv, shape, dtype):
    host = np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, 0x5A, np.uint8).view(dtype).reshape(shape)
    return mv.DeviceArray.from_host(host), host


def sweep(mv, svo, call, arrays, least):
    """`call` once for the number of allocations, then with each of them failing in turn; arrays: [(device, canary)] the call writes"""
    octree, info, state = svo.download(want_morton=True), bytes(svo.info()), mv.allocation_state()
    result = call()
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
        assert bytes(svo.info()) == info and all(np.array_equal(a, b) for a, b in zip(svo.download(want_morton=True), octree)), k
        for d, h in arrays:
            assert np.array_equal(d.to_host().view(np.uint8), h.view(np.uint8)), k  # the caller's arrays are written behind every allocation
    assert call() == result
    return total, result


def test_each_allocation_of_the_exterior_masks_fails_in_turn(mv, voxels):
    xyz, want = voxels
    assert want["nHidden"] > 1000
    svo = mv.IntersectorOctreeGPU()
    svo.build_voxels(xyz, None, origin=LOWER, dps=DPS, gridRes=RES)
    masks, host = filled(mv, len(want["masks"]), np.uint8)
    # region counter, keys, sorted keys, sort storage, parents, face counters
    total, result = sweep(mv, svo, lambda: svo.surface_exterior_masks_device(masks), [(masks, host)], 6)
    print("exterior masks: allocations failed in turn:", total)
    assert result == (want["nFaces"], want["nHidden"]) and np.array_equal(masks.to_host(), want["masks"])
    total, result = sweep(mv, svo, svo.surface_exterior_masks_device, [], 7)  # counts only: and the masks of its own
    assert result == (want["nFaces"], want["nHidden"])


def test_each_allocation_of_the_masked_quads_fails_in_turn(mv, voxels):
    xyz, want = voxels
    svo = mv.IntersectorOctreeGPU()
    svo.build_voxels(xyz, None, origin=LOWER, dps=DPS, gridRes=RES)
    ext = mv.DeviceArray.from_host(want["masks"])
    n = want["nFaces"]
    arrays = [filled(mv, n, np.uint32), filled(mv, n, np.uint8), filled(mv, (n, 4, 3), np.float32)]
    (fv, _), (fd, _), (pos, _) = arrays
    # masks scratch, counter, offsets, scan storage
    total, result = sweep(mv, svo, lambda: svo.surface_quads_device(n, fv, fd, pos, masks=ext), arrays, 4)
    print("masked quads: allocations failed in turn:", total)
    want_fv, want_fd, corners = S.faces(want["xyz"], want["masks"])
    assert result == n and np.array_equal(fv.to_host(), want_fv) and np.array_equal(fd.to_host(), want_fd)
    assert np.array_equal(pos.to_host().view(np.uint32), S.positions(corners, LOWER, DPS).view(np.uint32))
    assert np.array_equal(ext.to_host(), want["masks"])  # the given masks are only read
