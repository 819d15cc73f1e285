"""The voxel set as a numpy model of the last-wins edit semantics (mvrt_svo_edit_voxels), and the check that a handle holds exactly the octree the oracle builds
over a voxel list: what tests/test_gpu_voxel_edit.py, tests/test_gpu_walk.py, their alloc-failure sweeps and tests/test_gpu_deep_octree.py share."""
import numpy as np

SET, REMOVE = 1, 0


def normalised(attrs):
    a = np.array(attrs, np.uint8).reshape(-1, 8)
    a[:, 3] = 255
    a[:, 7] = 255
    return a


def has_emission(attrs):
    return int(np.any(attrs[:, 4:7] != 0))


def oracle_octree(O, morton, grid_res, flags):
    return O.build_octree(morton, grid_res, dag=not (flags & 1), embed=not (flags & 2))


def assert_svo(O, svo, morton, attrs, he, grid_res, flags, dumped, nodes=None):
    """the handle holds exactly the octree the oracle builds over (morton, attrs)"""
    info = svo.info()
    if nodes is None:
        nodes = oracle_octree(O, morton, grid_res, flags)
    assert info.totalDumpedVoxels == dumped, ("totalDumpedVoxels", info.totalDumpedVoxels, dumped)
    assert info.numberOfVoxels == len(morton), ("numberOfVoxels", info.numberOfVoxels, len(morton))
    assert info.numberOfNodes == len(nodes), ("numberOfNodes", info.numberOfNodes, len(nodes))
    assert info.hasEmission == he, ("hasEmission", info.hasEmission, he)
    gn, ga, gm = svo.download(want_morton=True)
    assert np.array_equal(gm, morton), "morton"
    assert np.array_equal(ga, attrs), "attrs"
    got = gn.view(O.NODE_DTYPE)
    for f in ("mask", "children", "psum"):
        assert np.array_equal(got[f], nodes[f]), f


class Model:
    """the voxel set as a dict Morton -> attribute row, with the last-wins batch semantics"""

    def __init__(self, O, xyz, attrs):
        m, a, _ = O.merge_voxels(O.morton_encode_batch(xyz), attrs)
        self.d = {int(k): a[i] for i, k in enumerate(m)}

    def apply(self, O, xyz, attrs, ops):
        keys = O.morton_encode_batch(xyz)
        attrs = normalised(attrs)
        for i, k in enumerate(keys):
            if ops[i] == SET:
                self.d[int(k)] = attrs[i]
            else:
                self.d.pop(int(k), None)

    def arrays(self):
        ks = np.array(sorted(self.d), np.uint64)
        at = np.array([self.d[int(k)] for k in ks], np.uint8).reshape(-1, 8)
        return ks, at
