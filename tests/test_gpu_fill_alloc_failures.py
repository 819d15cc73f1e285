"""Every device allocation of mvrt_svo_enclosed_cells and mvrt_svo_fill_enclosed is made to fail in turn (mvrt_test_fail_allocation), like
tests/test_gpu_surface_alloc_failures.py does for the surface calls and tests/test_gpu_alloc_failures.py for the edits.  The listing only reads the handle: each
failure names the hook, leaves the octree bit-identical and the caller's arrays untouched, and mvrt_test_allocation_state returns to where it was.  The fill
follows the edit: up to the adoption of the new arrays a failure leaves the old octree whole, from there on an empty handle, and nothing leaks either way."""
import numpy as np
import pytest

import fill_expected as F
from alloc_sweep import filled, mv, same, sweep_edit, sweep_reader  # noqa: F401 (mv: the fixture)
from voxel_sets import DPS, LOWER

pytestmark = pytest.mark.gpu

RES = 32


@pytest.fixture(scope="module")
def voxels():
    rng = np.random.default_rng(31)
    xyz = np.argwhere(rng.random((RES, RES, RES)) < 0.7).astype(np.uint32)
    return xyz, F.enclosed(xyz, RES)


def build(mv, svo, xyz):
    svo.build_voxels(xyz, None, origin=LOWER, dps=DPS, gridRes=RES)


def test_each_allocation_of_the_listing_fails_in_turn(mv, voxels):
    xyz, want = voxels
    n = len(want["xyz"])
    assert n > 100
    svo = mv.IntersectorOctreeGPU()
    build(mv, svo, xyz)
    (dx, hx), (dr, hr) = filled(mv, (n, 3), np.uint32), filled(mv, n, np.uint32)
    # counter, keys, sorted keys, sort storage, parents, offsets, scan storage; pairs twice, sort storage, first cells, ranks, scan storage
    total, result = sweep_reader(mv, lambda: svo.enclosed_cells_device(n, dx, dr), [svo], ((dx, hx), (dr, hr)), 14)
    print("listing: allocations failed in turn:", total)
    assert result == (n, want["nRegions"])
    assert np.array_equal(dx.to_host(), want["xyz"]) and np.array_equal(dr.to_host(), want["region"])


def test_each_allocation_of_the_fill_fails_in_turn(mv, voxels):
    xyz, want = voxels
    n = len(want["xyz"])
    glow = np.array([9, 8, 7, 255, 6, 0, 0, 255], np.uint8)
    twin = mv.IntersectorOctreeGPU()
    build(mv, twin, xyz)
    twin.edit_voxels(want["xyz"], np.tile(glow, (n, 1)))
    expected = twin.download(want_morton=True)
    base = mv.allocation_state()[:2]
    svo = mv.IntersectorOctreeGPU()
    build(mv, svo, xyz)

    def call():
        assert svo.fill_enclosed(glow) == n

    total, kept = sweep_edit(mv, call, svo, lambda: build(mv, svo, xyz), base, svo.enclosed_cells_device, 20)
    print("fill: allocations failed in turn:", total, "-- old octree kept by the first", kept)
    assert same(svo.download(want_morton=True), expected)
