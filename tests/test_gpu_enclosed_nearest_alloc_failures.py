"""Every device allocation of mvrt_svo_enclosed_nearest and mvrt_svo_fill_enclosed_nearest is made to fail in turn (mvrt_test_fail_allocation), like
tests/test_gpu_fill_alloc_failures.py does for the plain fill, on the 32^3 block among noise of tests/test_gpu_ball_alloc_failures.py with the block hollowed out.
The listing only reads the handle: each failure names the hook, leaves the octree bit-identical and the caller's arrays untouched, and
mvrt_test_allocation_state returns to where it was.  The fill follows the edit: up to the adoption of the new arrays a failure leaves the old octree whole, from
there on an empty handle, and nothing leaks either way."""
import numpy as np
import pytest

import nearest_expected as N
from alloc_sweep import filled, mv, same, sweep_edit, sweep_reader  # noqa: F401 (mv: the fixture)
from voxel_sets import DPS, LOWER

pytestmark = pytest.mark.gpu

RES = 32
KEYS = ("xyz", "region", "dist2", "nearest", "attribs")


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


def test_each_allocation_of_the_listing_fails_in_turn(mv, voxels):
    xyz, at, want = voxels
    n = len(want["xyz"])
    assert n > 900
    svo = mv.IntersectorOctreeGPU()
    build(svo, xyz, at)
    shapes = {"xyz": ((n, 3), np.uint32), "region": (n, np.uint32), "dist2": (n, np.uint32), "nearest": (n, np.uint32), "attribs": ((n, 8), np.uint8)}
    arrays = {k: filled(mv, *shapes[k]) for k in KEYS}
    dev = {k: arrays[k][0] for k in KEYS}
    # the classification's 7, the counters and the x pass's 4, per pass the sort's 3 and 8 more, the last sort's 3, roots, first cells, ranks, scan storage
    total, result = sweep_reader(mv, lambda: svo.enclosed_nearest_device(n, **dev), [svo], list(arrays.values()), 40)
    print("listing: allocations failed in turn:", total)
    assert result == (n, want["nRegions"])
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

    def call():
        assert svo.fill_enclosed_nearest() == n

    total, kept = sweep_edit(mv, call, svo, lambda: build(svo, xyz, at), base, svo.enclosed_nearest_device, 40)
    print("fill: allocations failed in turn:", total, "-- old octree kept by the first", kept)
    assert same(svo.download(want_morton=True), expected)
