"""Every device allocation of mvrt_svo_surface_merged is made to fail in turn (mvrt_test_fail_allocation), with and without the weld flag, like
tests/test_gpu_surface_alloc_failures.py does for the three other surface calls.  The call only reads the handle and keeps its scratch in DevBufs: each
failure is an error that names the hook, leaves the octree bit-identical and the caller's arrays untouched, and mvrt_test_allocation_state returns to where
it was; the same call without the hook then gives the model's result."""
import numpy as np
import pytest

import merge_expected as M
import surface_expected as S

pytestmark = pytest.mark.gpu

LOWER, DPS, RES = np.array([-0.3, 0.7, 1.1], np.float32), np.float32(0.013), 32


@pytest.fixture(scope="module")
def mv():
    import massivevoxelraytracing_amd as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def scene(mv):
    rng = np.random.default_rng(21)
    xyz = S.sorted_voxels(np.argwhere(rng.random((RES, RES, RES)) < 0.2))
    attrs = np.array([(200, 10, 10, 255, 0, 0, 0, 255), (10, 10, 200, 255, 0, 0, 0, 255)], np.uint8)[rng.integers(0, 2, size=len(xyz))]
    svo = mv.IntersectorOctreeGPU()
    svo.build_voxels(xyz.astype(np.uint32), attrs, origin=LOWER, dps=DPS, gridRes=RES)
    got_xyz, attrs = svo.read_voxels()  # the model runs on the bytes the build stored
    assert np.array_equal(got_xyz, xyz) and len(np.unique(attrs.view(np.uint64))) == 2
    return svo, xyz, attrs


def filled(mv, shape, dtype):
    host = np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, 0x5A, np.uint8).view(dtype).reshape(shape)
    return mv.DeviceArray.from_host(host), host


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("flags", [0, M.WELD])
def test_each_allocation_fails_in_turn(mv, scene, flags):
    svo, xyz, attrs = scene
    want = M.merged(xyz, attrs, RES, LOWER, DPS, flags)
    n, m = len(want["rectVoxel"]), len(want["vertices"]) if flags else 0
    shapes = {"rectVoxel": (n, np.uint32), "rectDir": (n, np.uint8), "rectSize": ((n, 2), np.uint32), "positions": ((n, 4, 3), np.float32)}
    if flags:
        shapes.update(indices=((n, 4), np.uint32), vertices=((m, 3), np.float32))
    outs = {k: filled(mv, s, t) for k, (s, t) in shapes.items()}
    d = {k: v[0] for k, v in outs.items()}

    def call():
        return svo.surface_merged_device(flags, n, m, **d)

    octree = svo.download(want_morton=True)
    info = bytes(svo.info())
    state = mv.allocation_state()
    assert call() == (want["nFaces"], n, m)
    total = mv.allocation_state()[2] - state[2]
    # the counter and the masks; per direction offsets, two sorts, two head scans and the rectangles, each with library storage; + keys, values (twice), ranks
    assert total >= 2 + 6 * 16 + (7 if flags else 0)
    assert mv.allocation_state()[:2] == state[:2]
    for k in d:  # back to the canary for the sweep
        mv.lib().mvrt_memcpy_h2d(d[k].ptr, outs[k][1].ctypes.data, d[k].nbytes, None)
    for k in range(1, total + 1):
        mv.set_test_fail_allocation(k)
        with pytest.raises(mv.MvrtError, match="mvrt_test_fail_allocation"):
            call()
        assert mv.lib().mvrt_test_fail_allocation(0) == 0
        assert mv.allocation_state()[:2] == state[:2], k  # nothing leaked
        assert bytes(svo.info()) == info and all(np.array_equal(a, b) for a, b in zip(svo.download(want_morton=True), octree)), k
        for name in d:  # the caller's arrays are written last, behind every allocation
            assert np.array_equal(bits(d[name].to_host()), bits(outs[name][1])), (k, name)
    print("flags", flags, "allocations failed in turn:", total)
    call()
    for name in d:
        assert np.array_equal(bits(d[name].to_host()), bits(want[name])), name
