"""Every device allocation of mvrt_svo_lod_prepare is made to fail in turn (mvrt_test_fail_allocation), through tests/alloc_sweep.py as for the other operators.
The call only adds to the handle: each failure names the hook, leaves the octree whole -- the same download and the same read_voxels -- and no pyramid, half-built
or old, and mvrt_test_allocation_state returns to where it was without a pyramid."""
import numpy as np
import pytest

import coarsen_expected as X
import surface_expected as S
from alloc_sweep import fail_kth, mv, sweep_reader, with_morton  # noqa: F401 (mv: the fixture)
from voxel_sets import DPS, LOWER

pytestmark = pytest.mark.gpu

RES, LEVELS = 32, 5


@pytest.fixture(scope="module")
def voxels():
    rng = np.random.default_rng(52)
    xyz = np.argwhere(rng.random((RES, RES, RES)) < 0.2).astype(np.uint32)
    return xyz, rng.integers(0, 256, size=(len(xyz), 8), dtype=np.uint8)


def whole(handle):
    return with_morton(handle) + tuple(handle.read_voxels())


@pytest.mark.parametrize("flags", [0, 2])
def test_each_allocation_of_the_pyramid_fails_in_turn(mv, voxels, flags):
    xyz, attribs = voxels
    svo = mv.IntersectorOctreeGPU()
    svo.build_voxels(xyz, attribs, origin=LOWER, dps=DPS, gridRes=RES, flags=flags)

    def no_pyramid():  # before every failing call and behind the last one: the call before has left nothing
        assert svo.lod_bytes() == 0
        with pytest.raises(mv.MvrtError, match="no attribute pyramid"):
            svo.lod_view()

    def prepare_and_release():  # (released so that the tallies of a success compare with those of a failure)
        nbytes = svo.lod_prepare()
        svo.lod_release()
        return nbytes

    # per level: ranks, scan storage, sums, counts, codes, attributes
    total, nbytes = sweep_reader(mv, prepare_and_release, [svo], [], 6 * (LEVELS - 1), reset=no_pyramid, download=whole)
    print("lod_prepare, flags", flags, ": allocations failed in turn:", total, "-- pyramid bytes", nbytes)
    assert nbytes == sum(len(X.coarse(xyz, attribs, k)["count"]) for k in range(1, LEVELS)) * 20

    # the same with a pyramid in place before every call: it goes first and stays gone, the octree is whole, nothing leaks
    snap, bare = whole(svo), mv.allocation_state()[:2]
    for k in range(1, total + 1):
        assert svo.lod_prepare() == nbytes
        fail_kth(mv, k, svo.lod_prepare)
        no_pyramid()
        assert mv.allocation_state()[:2] == bare, k
        assert all(np.array_equal(a, b) for a, b in zip(whole(svo), snap)), k
    svo.lod_prepare()
    lv, want = svo.lod_level(LEVELS - 1), X.coarse(xyz, attribs, 1)
    assert np.array_equal(lv["code"], S.morton(want["xyz"].astype(np.int64))) and np.array_equal(lv["attribs"], want["attribs"]) and np.array_equal(lv["count"], want["count"])
