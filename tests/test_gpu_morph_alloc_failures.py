"""Every device allocation of the six morphology calls is made to fail in turn (mvrt_test_fail_allocation), like tests/test_gpu_fill_alloc_failures.py does for
the fill.  The listings only read the handle: each failure names the hook, leaves the octree bit-identical and the caller's arrays untouched, and
mvrt_test_allocation_state returns to where it was.  The in-place calls follow the edit: up to the adoption of the new arrays a failure leaves the old octree
whole, from there on an empty handle, and nothing leaks either way."""
import numpy as np
import pytest

import morph_expected as M
from alloc_sweep import filled, mv, same, sweep_edit, sweep_reader  # noqa: F401 (mv: the fixture)
from voxel_sets import DPS, LOWER, block_and_noise

pytestmark = pytest.mark.gpu

RES = 32


@pytest.fixture(scope="module")
def voxels():
    return block_and_noise(31, RES)


def build(svo, voxels):
    svo.build_voxels(voxels[0], voxels[1], origin=LOWER, dps=DPS, gridRes=RES)


def test_each_allocation_of_the_listings_fails_in_turn(mv, voxels):
    svo = mv.IntersectorOctreeGPU()
    build(svo, voxels)
    x0, a0 = svo.read_voxels()
    want = M.dilation_cells(x0, a0, RES, M.CUBE)
    gone = M.erosion_voxels(x0, RES, M.CUBE)
    n, m = len(want["xyz"]), len(gone)
    assert n > 100 and m > 100
    (dx, hx), (da, ha), (dc, hc), (dv, hv) = filled(mv, (n, 3), np.uint32), filled(mv, (n, 8), np.uint8), filled(mv, n, np.uint32), filled(mv, m, np.uint32)
    calls = ((lambda: svo.dilation_cells_device(M.CUBE, n, dx, da, dc), n, 9, ((dx, hx), (da, ha), (dc, hc))),  # masks, offsets, scan storage, pairs twice, sort storage, ranks, ...
             (lambda: svo.erosion_voxels_device(M.CUBE, m, dv), m, 3, ((dv, hv),)))  # masks, offsets, scan storage
    for call, count, least, arrays in calls:
        total, result = sweep_reader(mv, call, [svo], arrays, least)
        print("listing: allocations failed in turn:", total)
        assert result == count
    assert np.array_equal(dx.to_host(), want["xyz"]) and np.array_equal(da.to_host(), want["attribs"]) and np.array_equal(dc.to_host(), want["count"])
    assert np.array_equal(dv.to_host(), gone)


@pytest.mark.parametrize("op,element,steps", [("dilate", M.FACES, 1), ("erode", M.CUBE, 1), ("close", M.CUBE, 2), ("open", M.FACES, 1)])
def test_each_allocation_of_an_in_place_call_fails_in_turn(mv, voxels, op, element, steps):
    base = mv.allocation_state()[:2]
    svo = mv.IntersectorOctreeGPU()
    build(svo, voxels)
    x0, a0 = svo.read_voxels()
    wx, wa = M.morph(op, x0, a0, RES, element, steps)

    def call():
        assert getattr(svo, op)(element, steps) == abs(len(wx) - len(x0)) > 0

    total, kept = sweep_edit(mv, call, svo, lambda: build(svo, voxels), base, svo.dilation_cells_device, 10)
    print(op, "allocations failed in turn:", total, "-- old octree kept by the first", kept)
    assert same(svo.read_voxels(), (wx, wa))
