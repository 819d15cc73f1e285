"""Every device allocation of the three surface calls is made to fail in turn (mvrt_test_fail_allocation), like tests/test_gpu_alloc_failures.py does for
the calls that make octrees.  The surface calls only read the handle and keep their scratch in DevBufs: each failure is an error that names the hook,
leaves the octree bit-identical and the caller's arrays untouched, and mvrt_test_allocation_state returns to where it was; the same call without the hook
then gives the model's result."""
import numpy as np
import pytest

import surface_expected as S
from alloc_sweep import bits, filled, mv, sweep_reader  # noqa: F401 (mv: the fixture)
from voxel_sets import DPS, LOWER

pytestmark = pytest.mark.gpu

RES = 32


@pytest.fixture(scope="module")
def scene(mv):
    rng = np.random.default_rng(21)
    xyz = np.argwhere(rng.random((RES, RES, RES)) < 0.2)
    svo = mv.IntersectorOctreeGPU()
    svo.build_voxels(xyz.astype(np.uint32), None, origin=LOWER, dps=DPS, gridRes=RES)
    return svo, S.surface(xyz, RES, LOWER, DPS)


@pytest.mark.parametrize("which", ["masks", "quads", "mesh"])
def test_each_allocation_fails_in_turn(mv, scene, which):
    svo, want = scene
    n, m = want["nFaces"], len(want["vertices"])
    outs = {"masks": filled(mv, len(want["xyz"]), np.uint8), "faceVoxel": filled(mv, n, np.uint32), "faceDir": filled(mv, n, np.uint8),
            "positions": filled(mv, (n, 4, 3), np.float32), "indices": filled(mv, (n, 4), np.uint32), "vertices": filled(mv, (m, 3), np.float32)}
    d = {k: v[0] for k, v in outs.items()}
    call = {"masks": lambda: svo.surface_masks_device(d["masks"]),
            "quads": lambda: svo.surface_quads_device(n, d["faceVoxel"], d["faceDir"], d["positions"]),
            "mesh": lambda: svo.surface_mesh_device(n, m, d["faceVoxel"], d["faceDir"], d["indices"], d["vertices"])}[which]
    used = {"masks": ("masks",), "quads": ("faceVoxel", "faceDir", "positions"), "mesh": ("faceVoxel", "faceDir", "indices", "vertices")}[which]
    # the counter; + masks, offsets, scan storage; + keys, values (twice), sort storage, ranks, scan storage
    total, _ = sweep_reader(mv, call, [svo], [outs[name] for name in used], {"masks": 1, "quads": 4, "mesh": 10}[which])
    print(which, "allocations failed in turn:", total)
    for name in used:
        assert np.array_equal(bits(d[name].to_host()), bits(want[name])), name
