"""Every device allocation of the three surface calls is made to fail in turn (mvrt_test_fail_allocation), like tests/test_gpu_alloc_failures.py does for
the calls that make octrees.  The surface calls only read the handle and keep their scratch in DevBufs: each failure is an error that names the hook,
leaves the octree bit-identical and the caller's arrays untouched, and mvrt_test_allocation_state returns to where it was; the same call without the hook
then gives the model's result."""
import numpy as np
import pytest

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
    xyz = np.argwhere(rng.random((RES, RES, RES)) < 0.2)
    svo = mv.IntersectorOctreeGPU()
    svo.build_voxels(xyz.astype(np.uint32), None, origin=LOWER, dps=DPS, gridRes=RES)
    return svo, S.surface(xyz, RES, LOWER, DPS)


def filled(mv, shape, dtype):
    host = np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, 0x5A, np.uint8).view(dtype).reshape(shape)
    return mv.DeviceArray.from_host(host), host


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("which", ["masks", "quads", "mesh"])
def test_each_allocation_fails_in_turn(mv, scene, which):
    svo, want = scene
    n, m = want["nFaces"], len(want["vertices"])
    outs = {"masks": filled(mv, len(want["xyz"]), np.uint8), "faceVoxel": filled(mv, n, np.uint32), "faceDir": filled(mv, n, np.uint8),
            "positions": filled(mv, (n, 4, 3), np.float32), "indices": filled(mv, (n, 4), np.uint32), "vertices": filled(mv, (m, 3), np.float32)}
    d = {k: v[0] for k, v in outs.items()}
    call = {"masks": lambda: svo.surface_masks_device(d["masks"]),
            "quads": lambda: svo.surface_quads_device(n, d["faceVoxel"], d["faceDir"], d["positions"]),
            "mesh": lambda: svo.surface_mesh_device(n, m, d["faceVoxel"], d["faceDir"], d["indices"], d["vertices"])}[which]
    used = {"masks": ("masks",), "quads": ("faceVoxel", "faceDir", "positions"), "mesh": ("faceVoxel", "faceDir", "indices", "vertices")}[which]
    octree = svo.download(want_morton=True)
    info = bytes(svo.info())
    state = mv.allocation_state()
    call()
    total = mv.allocation_state()[2] - state[2]
    assert total >= {"masks": 1, "quads": 4, "mesh": 10}[which]  # the counter; + masks, offsets, scan storage; + keys, values (twice), sort storage, ranks, scan storage
    assert mv.allocation_state()[:2] == state[:2]
    for k in used:  # back to the canary for the sweep
        mv.lib().mvrt_memcpy_h2d(d[k].ptr, outs[k][1].ctypes.data, d[k].nbytes, None)
    for k in range(1, total + 1):
        mv.set_test_fail_allocation(k)
        with pytest.raises(mv.MvrtError, match="mvrt_test_fail_allocation"):
            call()
        assert mv.lib().mvrt_test_fail_allocation(0) == 0
        assert mv.allocation_state()[:2] == state[:2], k  # nothing leaked
        assert bytes(svo.info()) == info and all(np.array_equal(a, b) for a, b in zip(svo.download(want_morton=True), octree)), k
        for name in used:  # the caller's arrays are written last, behind every allocation
            assert np.array_equal(bits(d[name].to_host()), bits(outs[name][1])), (k, name)
    print(which, "allocations failed in turn:", total)
    call()
    got = {name: d[name].to_host() for name in used}
    for name in used:
        assert np.array_equal(bits(got[name]), bits(want[name])), name
