"""Every device allocation of the two component calls is made to fail in turn (mvrt_test_fail_allocation), like tests/test_gpu_morph_alloc_failures.py does for the
morphology.  The listing only reads the handle: each failure names the hook, leaves the octree bit-identical and the caller's arrays untouched, and
mvrt_test_allocation_state returns to where it was.  The in-place call follows the edit: up to the adoption of the new arrays a failure leaves the old octree
whole, from there on an empty handle, and nothing leaks either way."""
import numpy as np
import pytest

import components_expected as K
from alloc_sweep import filled, mv, same, sweep_edit, sweep_reader  # noqa: F401 (mv: the fixture)
from voxel_sets import DPS, LOWER, block_and_noise

pytestmark = pytest.mark.gpu

RES = 32


@pytest.fixture(scope="module")
def voxels():
    return block_and_noise(31, RES)


def build(svo, voxels):
    svo.build_voxels(voxels[0], voxels[1], origin=LOWER, dps=DPS, gridRes=RES)


@pytest.mark.parametrize("element", [K.FACES, K.CUBE])
def test_each_allocation_of_the_listing_fails_in_turn(mv, voxels, element):
    svo = mv.IntersectorOctreeGPU()
    build(svo, voxels)
    x0, _ = svo.read_voxels()
    want = K.components(x0, RES, element)
    n, big = len(want["size"]), int(want["size"].max())
    assert n > 100
    (dl, hl), (ds, hs), (df, hf), (db, hb) = filled(mv, len(x0), np.uint32), filled(mv, n, np.uint32), filled(mv, n, np.uint32), filled(mv, (n, 6), np.uint32)
    arrays = ((dl, hl), (ds, hs), (df, hf), (db, hb))
    # parents, ranks, scan storage, sizes, boxes, the largest
    total, result = sweep_reader(mv, lambda: svo.components_device(element, dl, n, ds, df, db), [svo], arrays, 6)
    print("listing: allocations failed in turn:", total)
    assert result == (n, big)
    assert np.array_equal(dl.to_host(), want["label"]) and np.array_equal(ds.to_host(), want["size"])
    assert np.array_equal(df.to_host(), want["first"]) and np.array_equal(db.to_host(), want["box"])


@pytest.mark.parametrize("element,min_voxels,keep_largest", [(K.FACES, 2, 0), (K.CUBE, 1, 1)])
def test_each_allocation_of_the_in_place_call_fails_in_turn(mv, voxels, element, min_voxels, keep_largest):
    base = mv.allocation_state()[:2]
    svo = mv.IntersectorOctreeGPU()
    build(svo, voxels)
    x0, a0 = svo.read_voxels()
    wx, wa = K.keep(x0, a0, RES, element, min_voxels, keep_largest)

    def call():
        assert svo.keep_components(element, min_voxels, keep_largest)[0] == len(x0) - len(wx) > 0

    total, kept = sweep_edit(mv, call, svo, lambda: build(svo, voxels), base, svo.components_device, 10)
    print("keep_components: allocations failed in turn:", total, "-- old octree kept by the first", kept)
    assert same(svo.read_voxels(), (wx, wa))
