"""Every device allocation of mvrt_svo_coarse_voxels and mvrt_svo_coarsen is made to fail in turn (mvrt_test_fail_allocation), like
tests/test_gpu_fill_alloc_failures.py does for the fill.  The listing only reads the handle: each failure names the hook, leaves the octree bit-identical and the
caller's arrays untouched, and mvrt_test_allocation_state returns to where it was.  The build follows the voxel-list build: up to the adoption of the new arrays a
failure leaves the destination as it was, from there on empty; the source, where it is another handle, stays whole; nothing leaks either way."""
import numpy as np
import pytest

import coarsen_expected as X
from alloc_sweep import filled, mv, same, sweep_edit, sweep_reader  # noqa: F401 (mv: the fixture)
from voxel_sets import DPS, LOWER

pytestmark = pytest.mark.gpu

RES = 32


@pytest.fixture(scope="module")
def voxels():
    rng = np.random.default_rng(51)
    xyz = np.argwhere(rng.random((RES, RES, RES)) < 0.2).astype(np.uint32)
    return xyz, rng.integers(0, 256, size=(len(xyz), 8), dtype=np.uint8)


def build(svo, xyz, attribs, res=RES):
    svo.build_voxels(xyz, attribs, origin=LOWER, dps=DPS, gridRes=res)


@pytest.mark.parametrize("min_count", [1, 2])
def test_each_allocation_of_the_listing_fails_in_turn(mv, voxels, min_count):
    xyz, attribs = voxels
    want = X.coarse(xyz, attribs, 1, min_count)
    n = len(want["xyz"])
    assert n > 1000
    svo = mv.IntersectorOctreeGPU()
    build(svo, xyz, attribs)
    arrays = [filled(mv, (n, 3), np.uint32), filled(mv, (n, 8), np.uint8), filled(mv, n, np.uint32)]
    args = (1, min_count, n) + tuple(d for d, _ in arrays)
    # ranks, scan storage, sums, counts, codes; with a minCount also the places of the kept cells and their scan storage
    total, result = sweep_reader(mv, lambda: svo.coarse_voxels_device(*args), [svo], arrays, 5 if min_count == 1 else 7)
    print("listing, minCount", min_count, ": allocations failed in turn:", total)
    assert result == n
    assert all(np.array_equal(d.to_host(), want[f]) for (d, _), f in zip(arrays, ("xyz", "attribs", "count")))


@pytest.mark.parametrize("in_place", [False, True])
def test_each_allocation_of_the_build_fails_in_turn(mv, voxels, in_place):
    xyz, attribs = voxels
    want = X.coarse(xyz, attribs, 1, 2)
    twin = mv.IntersectorOctreeGPU()
    twin.build_voxels(want["xyz"], want["attribs"], origin=LOWER, dps=np.float32(DPS * np.float32(2)), gridRes=RES // 2)
    expected = twin.download(want_morton=True)
    old_xyz = np.argwhere(np.ones((4, 4, 4), bool)).astype(np.uint32)  # what the destination holds before, where it is another handle
    base = mv.allocation_state()[:2]
    src, other = mv.IntersectorOctreeGPU(), mv.IntersectorOctreeGPU()
    dst = src if in_place else other

    def build_other():
        if not in_place:
            build(other, old_xyz, None, 4)

    def reset():
        build(src, xyz, attribs)
        build_other()

    build(src, xyz, attribs)
    held_by_source = tuple(a - b for a, b in zip(mv.allocation_state()[:2], base))  # (the destination is still empty here: what the source alone holds)
    build_other()
    total, kept = sweep_edit(mv, lambda: src.coarsen(1, 2, 0, dst), dst, reset, base, lambda: dst.coarse_voxels_device(1), 15,
                             bystanders=() if in_place else [src], live_when_empty=(0, 0) if in_place else held_by_source)
    print("coarsen, in place" if in_place else "coarsen", ": allocations failed in turn:", total, "-- old octree kept by the first", kept)
    assert same(dst.download(want_morton=True), expected)
