"""Every device allocation of mvrt_svo_surface_smooth is made to fail in turn (mvrt_test_fail_allocation), like tests/test_gpu_surface_alloc_failures.py does
for the calls it is built on.  The call only reads the handle and keeps its scratch in DevBufs: each failure is an error that names the hook, leaves the octree
bit-identical and the caller's six arrays untouched, and mvrt_test_allocation_state returns to where it was; the same call without the hook then gives the
model's result."""
import numpy as np
import pytest

import smooth_expected as M
from alloc_sweep import bits, filled, mv, sweep_reader  # noqa: F401 (mv: the fixture)
from voxel_sets import DPS, LOWER, build

pytestmark = pytest.mark.gpu


def test_each_allocation_fails_in_turn(mv):
    xyz = M.ball(16, 6.3)
    want = M.smooth(xyz, 16, LOWER, DPS, 2)
    svo = build(mv, xyz, 16)
    n, m = len(want["faceVoxel"]), len(want["corners"])
    names = ("faceVoxel", "faceDir", "indices", "vertices", "displacements", "neighbours")
    outs = [filled(mv, s, t) for s, t in ((n, np.uint32), (n, np.uint8), ((n, 4), np.uint32), ((m, 3), np.float32), ((m, 3), np.int32), (m, np.uint8))]
    p = mv.SmoothParams(iterations=2, weightEven=256, weightOdd=256, limit=127)
    # the mesh's ten (counter, masks, offsets, scan storage, keys and values twice, sort storage, ranks, scan storage), then the table, the mask, the corner
    # keys, the two displacement buffers and the clamp counter
    total, result = sweep_reader(mv, lambda: svo.surface_smooth_device(p, n, m, *[d for d, _ in outs]), [svo], outs, 16)
    print("smooth: allocations failed in turn:", total)
    assert result == (n, m, want["clamped"])
    for name, (d, _) in zip(names, outs):
        assert np.array_equal(bits(d.to_host()), bits(want[name])), name
    total, result = sweep_reader(mv, lambda: svo.surface_smooth_device(p, 0, m, displacements=outs[4][0]), [svo], [outs[4]], 18)  # and faceDir and indices of its own
    assert result == (n, m, want["clamped"]) and np.array_equal(outs[4][0].to_host(), want["displacements"])
