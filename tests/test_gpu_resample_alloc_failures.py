"""Every device allocation of the two resampling calls is made to fail in turn (mvrt_test_fail_allocation), like tests/test_gpu_combine_alloc_failures.py does for
the two-set calls.  The listing only reads the handle: each failure names the hook, leaves the octree bit-identical and the caller's arrays untouched, and
mvrt_test_allocation_state returns to where it was.  The build follows the voxel-list build, as mvrt.h says: up to the adoption of the new arrays a failure leaves
dst bit-identical to what it was, from there on (the derived tables, made after the old octree is released) an empty handle; src stays bit-identical and nothing
leaks either way."""
import numpy as np
import pytest

import resample_expected as E
from alloc_sweep import filled, mv, same, sweep_edit, sweep_reader  # noqa: F401 (mv: the fixture)
from voxel_sets import DPS, LOWER, block_and_noise

pytestmark = pytest.mark.gpu

RES = 32
TURN = E.rotation((1, 2, 3), 30.0)


def build(svo, v, res=RES):
    svo.build_voxels(v[0], v[1], origin=LOWER, dps=DPS, gridRes=res)


@pytest.mark.parametrize("rd", [32, 64])
def test_each_allocation_of_the_listing_fails_in_turn(mv, rd):
    src = mv.IntersectorOctreeGPU()
    build(src, block_and_noise(31, RES))
    mt = E.about_centre(TURN * (RES / rd), RES, rd)
    xf = mv.CellTransform.make(*mt)
    want = E.dense(*src.read_voxels(), RES, mt[0], mt[1], rd)
    n = len(want["xyz"])
    assert n > 1000
    arrays = (filled(mv, (n, 3), np.uint32), filled(mv, (n, 8), np.uint8), filled(mv, n, np.uint32))
    call = lambda: src.resample_voxels_device(xf, rd, n, arrays[0][0], arrays[1][0], arrays[2][0])
    levels = rd.bit_length() - 1
    # the root; masks, offsets and scan storage per level; a frontier per level but the last
    total, result = sweep_reader(mv, call, [src], arrays, 1 + 3 * levels + (levels - 1))
    print("listing, Rd", rd, ": allocations failed in turn:", total)
    assert result == n
    assert all(np.array_equal(d.to_host(), want[key]) for (d, _), key in zip(arrays, ("xyz", "attribs", "source")))


@pytest.mark.parametrize("in_place", [False, True])
def test_each_allocation_of_the_build_fails_in_turn(mv, in_place):
    mt = E.about_centre(TURN, RES, RES)
    xf = mv.CellTransform.make(*mt)
    base = mv.allocation_state()[:2]
    src, dst = mv.IntersectorOctreeGPU(), mv.IntersectorOctreeGPU()
    v_src, v_dst = block_and_noise(31, RES), block_and_noise(35, RES)
    build(src, v_src)
    held_src = tuple(x - y for x, y in zip(mv.allocation_state()[:2], base))
    if in_place:
        dst, v_dst, held_src = src, v_src, (0, 0)
    else:
        build(dst, v_dst)
    want = E.dense(*src.read_voxels(), RES, mt[0], mt[1], RES)
    total, kept = sweep_edit(mv, lambda: src.resample(xf, dst), dst, lambda: build(dst, v_dst), base, lambda: dst.resample_voxels_device(xf, RES), 20,
                             bystanders=() if in_place else [src], live_when_empty=held_src)
    print("resample, in place", in_place, ": allocations failed in turn:", total, "-- old octree kept by the first", kept)
    assert kept >= 20  # every allocation of the refinement and of the levels keeps dst whole
    assert same(dst.read_voxels(), (want["xyz"], want["attribs"]))
