"""Every device allocation of the two combine calls is made to fail in turn (mvrt_test_fail_allocation), like tests/test_gpu_components_alloc_failures.py does for
the components, for a zero offset (b's codes as they are) and a non-zero one (translate, compact, sort).  The listing only reads the handles: each failure names
the hook, leaves both octrees bit-identical and the caller's arrays untouched, and mvrt_test_allocation_state returns to where it was.  The in-place call follows
the edit: up to the adoption of the new arrays a failure leaves the old octree whole, from there on an empty handle; b stays whole and nothing leaks either way."""
import numpy as np
import pytest

import combine_expected as E
from alloc_sweep import filled, mv, same, sweep_edit, sweep_reader  # noqa: F401 (mv: the fixture)
from voxel_sets import DPS, LOWER, block_and_noise

pytestmark = pytest.mark.gpu

RES = 32
OFFSETS = [None, (3, -2, 1)]


def build(svo, v):
    svo.build_voxels(v[0], v[1], origin=LOWER, dps=DPS, gridRes=RES)


@pytest.mark.parametrize("offset", OFFSETS)
def test_each_allocation_of_the_listing_fails_in_turn(mv, offset):
    a, b = mv.IntersectorOctreeGPU(), mv.IntersectorOctreeGPU()
    build(a, block_and_noise(31, RES))
    build(b, block_and_noise(32, RES))
    (xa, aa), (xb, ab) = a.read_voxels(), b.read_voxels()
    want = E.combine(xa, aa, xb, ab, RES, E.XOR, offset, E.ATTRIB_B)
    n, counts = len(want["xyz"]), (len(want["xyz"]), want["overlap"], want["clipped"])
    assert n > 1000 and want["overlap"] > 500
    arrays = (filled(mv, (n, 3), np.uint32), filled(mv, (n, 8), np.uint8), filled(mv, n, np.uint8))
    call = lambda: a.combine_voxels_device(b, E.XOR, offset, E.ATTRIB_B, n, arrays[0][0], arrays[1][0], arrays[2][0])
    # partner, state, offsets and scan storage per list; + keys, scan, compaction, sort
    total, result = sweep_reader(mv, call, [a, b], arrays, 8 if offset is None else 14)
    print("listing, offset", offset, ": allocations failed in turn:", total)
    assert result == counts
    assert all(np.array_equal(d.to_host(), want[key]) for (d, _), key in zip(arrays, ("xyz", "attribs", "source")))


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("op,flags", [(E.UNION, E.ATTRIB_B), (E.DIFFERENCE, 0)])
def test_each_allocation_of_the_in_place_call_fails_in_turn(mv, offset, op, flags):
    b = mv.IntersectorOctreeGPU()
    build(b, block_and_noise(32, RES))
    base = mv.allocation_state()[:2]
    a = mv.IntersectorOctreeGPU()
    va = block_and_noise(31, RES)
    build(a, va)
    (xa, aa), (xb, ab) = a.read_voxels(), b.read_voxels()
    want = E.combine(xa, aa, xb, ab, RES, op, offset, flags)

    def call():
        added, removed, clipped = a.combine(b, op, offset, flags)
        assert added + removed > 0 and clipped == want["clipped"]

    total, kept = sweep_edit(mv, call, a, lambda: build(a, va), base, lambda: a.combine_voxels_device(b, op), 12, bystanders=[b])
    print("combine op", op, "offset", offset, ": allocations failed in turn:", total, "-- old octree kept by the first", kept)
    assert same(a.read_voxels(), (want["xyz"], want["attribs"]))


def test_each_allocation_of_a_recolouring_fails_in_turn(mv):
    """the attribute-only call writes in place, behind its last allocation: every failure leaves the old bytes"""
    va = block_and_noise(31, RES)
    a, b = mv.IntersectorOctreeGPU(), mv.IntersectorOctreeGPU()
    build(a, va)
    build(b, (va[0], np.random.default_rng(33).integers(0, 256, (len(va[0]), 8), dtype=np.uint8)))  # the same cells in other colours
    _, result = sweep_reader(mv, lambda: a.combine(b, E.INTERSECTION, None, E.ATTRIB_B), [a, b], [], 8, reset=lambda: build(a, va))
    assert result == (0, 0, 0) and same(a.read_voxels(), b.read_voxels())
