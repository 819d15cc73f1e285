"""Every device allocation of the six round-offset calls is made to fail in turn (mvrt_test_fail_allocation), like tests/test_gpu_morph_alloc_failures.py does for
the morphology, on the same 32^3 block among noise, at radius2 = 5.  The listings only read the handle: each failure names the hook, leaves the octree
bit-identical and the caller's arrays untouched, and mvrt_test_allocation_state returns to where it was.  The in-place calls follow the edit: up to the adoption
of the new arrays a failure leaves the old octree whole, from there on an empty handle, and nothing leaks either way."""
import numpy as np
import pytest

import ball_expected as B
from alloc_sweep import filled, mv, same, sweep_edit, sweep_reader  # noqa: F401 (mv is a fixture)
from voxel_sets import DPS, LOWER, block_and_noise

pytestmark = pytest.mark.gpu

RES, RHO = 32, 5


@pytest.fixture(scope="module")
def voxels():
    return block_and_noise(31, RES)


def build(svo, voxels):
    svo.build_voxels(voxels[0], voxels[1], origin=LOWER, dps=DPS, gridRes=RES)


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
    # seed flags, offsets, scan storage, seeds twice, then per pass offsets, scan storage, records three times, sorted twice, sort storage, ranks, ...
    calls = ((lambda: svo.distance_cells_device(RHO, n, dx, dd, dn, da), n, 30, ((dx, hx), (dd, hd), (dn, hn), (da, ha))),
             (lambda: svo.depth_voxels_device(RHO, m, dv, dp), m, 30, ((dv, hv), (dp, hp))))
    for call, count, least, arrays in calls:
        total, result = sweep_reader(mv, call, [svo], arrays, least)
        print("listing: allocations failed in turn:", total)
        assert result == count
    assert np.array_equal(dx.to_host(), want["xyz"]) and np.array_equal(dd.to_host(), want["dist2"]) and np.array_equal(dn.to_host(), want["nearest"])
    assert np.array_equal(da.to_host(), want["attribs"]) and np.array_equal(dv.to_host(), gone["vIndex"]) and np.array_equal(dp.to_host(), gone["depth2"])


@pytest.mark.parametrize("op", ["dilate", "erode", "close", "open"])
def test_each_allocation_of_an_in_place_call_fails_in_turn(mv, voxels, op):
    base = mv.allocation_state()[:2]
    svo = mv.IntersectorOctreeGPU()
    build(svo, voxels)
    x0, a0 = svo.read_voxels()
    wx, wa = B.ball(op, x0, a0, RES, RHO)

    def call():
        assert getattr(svo, op + "_ball")(RHO) == abs(len(wx) - len(x0)) > 0

    total, kept = sweep_edit(mv, call, svo, lambda: build(svo, voxels), base, svo.distance_cells_device, 30)
    print(op, "allocations failed in turn:", total, "-- old octree kept by the first", kept)
    assert same(svo.read_voxels(), (wx, wa))
