"""Every device allocation of mvrt_svo_surface_exterior_masks and of mvrt_svo_surface_quads_masked is made to fail in turn (mvrt_test_fail_allocation), like
tests/test_gpu_fill_alloc_failures.py does for the listing.  Both calls only read the handle: each failure names the hook, leaves the octree bit-identical and
the caller's arrays untouched, mvrt_test_allocation_state returns to where it was, and the call succeeds again afterwards."""
import numpy as np
import pytest

import exterior_expected as E
import surface_expected as S
from alloc_sweep import filled, mv, sweep_reader  # noqa: F401 (mv: the fixture)
from voxel_sets import DPS, LOWER

pytestmark = pytest.mark.gpu

RES = 32


@pytest.fixture(scope="module")
def voxels():
    rng = np.random.default_rng(31)
    xyz = np.argwhere(rng.random((RES, RES, RES)) < 0.7).astype(np.uint32)
    return xyz, E.exterior(xyz, RES)


def test_each_allocation_of_the_exterior_masks_fails_in_turn(mv, voxels):
    xyz, want = voxels
    assert want["nHidden"] > 1000
    svo = mv.IntersectorOctreeGPU()
    svo.build_voxels(xyz, None, origin=LOWER, dps=DPS, gridRes=RES)
    masks, host = filled(mv, len(want["masks"]), np.uint8)
    # region counter, keys, sorted keys, sort storage, parents, face counters
    total, result = sweep_reader(mv, lambda: svo.surface_exterior_masks_device(masks), [svo], [(masks, host)], 6)
    print("exterior masks: allocations failed in turn:", total)
    assert result == (want["nFaces"], want["nHidden"]) and np.array_equal(masks.to_host(), want["masks"])
    total, result = sweep_reader(mv, svo.surface_exterior_masks_device, [svo], [], 7)  # counts only: and the masks of its own
    assert result == (want["nFaces"], want["nHidden"])


def test_each_allocation_of_the_masked_quads_fails_in_turn(mv, voxels):
    xyz, want = voxels
    svo = mv.IntersectorOctreeGPU()
    svo.build_voxels(xyz, None, origin=LOWER, dps=DPS, gridRes=RES)
    ext = mv.DeviceArray.from_host(want["masks"])
    n = want["nFaces"]
    arrays = [filled(mv, n, np.uint32), filled(mv, n, np.uint8), filled(mv, (n, 4, 3), np.float32)]
    (fv, _), (fd, _), (pos, _) = arrays
    # masks scratch, counter, offsets, scan storage
    total, result = sweep_reader(mv, lambda: svo.surface_quads_device(n, fv, fd, pos, masks=ext), [svo], arrays, 4)
    print("masked quads: allocations failed in turn:", total)
    want_fv, want_fd, corners = S.faces(want["xyz"], want["masks"])
    assert result == n and np.array_equal(fv.to_host(), want_fv) and np.array_equal(fd.to_host(), want_fd)
    assert np.array_equal(pos.to_host().view(np.uint32), S.positions(corners, LOWER, DPS).view(np.uint32))
    assert np.array_equal(ext.to_host(), want["masks"])  # the given masks are only read
