"""Every device allocation of mvrt_svo_surface_ao is made to fail in turn (mvrt_test_fail_allocation), like tests/test_gpu_surface_alloc_failures.py does for the
surface calls.  The bake only reads the handle and keeps its scratch (the direction table) in a DevBuf: each failure is an error that names the hook, leaves the
octree bit-identical and the caller's array untouched, and mvrt_test_allocation_state returns to where it was; the handle still traces and the same call without
the hook then gives the result of an undisturbed one.  mvrt_trace_batch_range allocates nothing."""
import numpy as np
import pytest

from alloc_sweep import filled, mv  # noqa: F401 (mv: the fixture)
from voxel_sets import DPS, LOWER

pytestmark = pytest.mark.gpu

RES = 32


def test_each_allocation_fails_in_turn(mv):
    rng = np.random.default_rng(21)
    svo = mv.IntersectorOctreeGPU()
    svo.build_voxels(np.argwhere(rng.random((RES, RES, RES)) < 0.2).astype(np.uint32), None, origin=LOWER, dps=DPS, gridRes=RES)
    q = svo.surface_quads()
    n = len(q["faceVoxel"])
    fv, fd = mv.DeviceArray.from_host(q["faceVoxel"]), mv.DeviceArray.from_host(q["faceDir"])
    out, canary = filled(mv, n, np.uint16)
    radius = np.float32(4) * DPS
    call = lambda: svo.surface_ao_device(n, fv, fd, 64, radius, out)
    ro = (LOWER + rng.random((2000, 3)) * DPS * RES).astype(np.float32)
    rd = (rng.random((2000, 3)) - 0.5).astype(np.float32)
    traced = svo.intersect_range(ro, rd, radius, want_descents=True)
    octree = svo.download(want_morton=True)
    info = bytes(svo.info())
    state = mv.allocation_state()
    call()
    want = out.to_host()
    assert (want <= 64).all() and len(np.unique(want)) > 8
    total = mv.allocation_state()[2] - state[2]
    assert total >= 1  # the direction table
    assert mv.allocation_state()[:2] == state[:2]
    state = mv.allocation_state()
    svo.intersect_range(ro[:10], rd[:10], radius)
    assert mv.allocation_state() == state  # the batch call makes no allocation of the library's own
    for k in range(1, total + 1):
        mv.lib().mvrt_memcpy_h2d(out.ptr, canary.ctypes.data, out.nbytes, None)
        mv.set_test_fail_allocation(k)
        with pytest.raises(mv.MvrtError, match="mvrt_test_fail_allocation"):
            call()
        assert mv.lib().mvrt_test_fail_allocation(0) == 0
        assert mv.allocation_state()[:2] == state[:2], k  # nothing leaked
        assert bytes(svo.info()) == info and all(np.array_equal(a, b) for a, b in zip(svo.download(want_morton=True), octree)), k
        assert np.array_equal(out.to_host(), canary), k  # the caller's array is written last, behind every allocation
        again = svo.intersect_range(ro, rd, radius, want_descents=True)  # the handle still traces
        assert all(np.array_equal(again[key], traced[key]) for key in traced), k
        call()  # a retry succeeds
        assert np.array_equal(out.to_host(), want), k
    print("allocations failed in turn:", total)
