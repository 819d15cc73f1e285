"""Every device allocation of mvrt_svo_surface_merged is made to fail in turn (mvrt_test_fail_allocation), with and without the weld flag, like
tests/test_gpu_surface_alloc_failures.py does for the three other surface calls.  The call only reads the handle and keeps its scratch in DevBufs: each
failure is an error that names the hook, leaves the octree bit-identical and the caller's arrays untouched, and mvrt_test_allocation_state returns to where
it was; the same call without the hook then gives the model's result."""
import numpy as np
import pytest

import merge_expected as M
import surface_expected as S
from alloc_sweep import bits, filled, mv, sweep_reader  # noqa: F401 (mv: the fixture)
from voxel_sets import DPS, LOWER

pytestmark = pytest.mark.gpu

RES = 32


@pytest.fixture(scope="module")
def scene(mv):
    rng = np.random.default_rng(21)
    xyz = S.sorted_voxels(np.argwhere(rng.random((RES, RES, RES)) < 0.2))
    attrs = np.array([(200, 10, 10, 255, 0, 0, 0, 255), (10, 10, 200, 255, 0, 0, 0, 255)], np.uint8)[rng.integers(0, 2, size=len(xyz))]
    svo = mv.IntersectorOctreeGPU()
    svo.build_voxels(xyz.astype(np.uint32), attrs, origin=LOWER, dps=DPS, gridRes=RES)
    got_xyz, attrs = svo.read_voxels()  # the model runs on the bytes the build stored
    assert np.array_equal(got_xyz, xyz) and len(np.unique(attrs.view(np.uint64))) == 2
    return svo, xyz, attrs


@pytest.mark.parametrize("flags", [0, M.WELD])
def test_each_allocation_fails_in_turn(mv, scene, flags):
    svo, xyz, attrs = scene
    want = M.merged(xyz, attrs, RES, LOWER, DPS, flags)
    n, m = len(want["rectVoxel"]), len(want["vertices"]) if flags else 0
    shapes = {"rectVoxel": (n, np.uint32), "rectDir": (n, np.uint8), "rectSize": ((n, 2), np.uint32), "positions": ((n, 4, 3), np.float32)}
    if flags:
        shapes.update(indices=((n, 4), np.uint32), vertices=((m, 3), np.float32))
    outs = {k: filled(mv, s, t) for k, (s, t) in shapes.items()}
    d = {k: v[0] for k, v in outs.items()}
    # the counter and the masks; per direction offsets, two sorts, two head scans and the rectangles, each with library storage; + keys, values (twice), ranks
    total, result = sweep_reader(mv, lambda: svo.surface_merged_device(flags, n, m, **d), [svo], list(outs.values()), 2 + 6 * 16 + (7 if flags else 0))
    print("flags", flags, "allocations failed in turn:", total)
    assert result == (want["nFaces"], n, m)
    for name in d:
        assert np.array_equal(bits(d[name].to_host()), bits(want[name])), name
