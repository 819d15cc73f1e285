"""The model of mvrt_svo_walk_voxels (tests/test_walk_cpu.py, tests/test_gpu_walk.py): upload_shapes.voxel_paths extended to carry the nVoxelsPSum sum.

Plain numpy on oracle.NODE_DTYPE arrays (the reference's 68-byte nodes, root last), independent of the library: every root-to-voxel path of an octree that
keeps upload rules 2 and 3, in ascending path order, with the sum of the stored nVoxelsPSum along it (uint32 arithmetic, what the traversal reports as
vIndex) and the path decoded as a Morton code (x = bit 0 of each 3-bit group).  A DAG is walked per path; reachable nodes of mask 0 end their path."""
import numpy as np

import deep_scenes as D
import upload_shapes as U


def walk(nodes, res, embedded):
    """-> (paths uint64 sorted, vIndex uint32 per path, xyz (n, 3) uint32)"""
    L = U.levels_of(res)
    cur_n = np.array([len(nodes) - 1], np.int64)
    cur_p = np.zeros(1, np.uint64)
    cur_s = np.zeros(1, np.uint64)
    for lvl in range(L):
        m = nodes["mask"][cur_n].astype(np.int64)
        ch = nodes["children"][cur_n].astype(np.int64)
        ps = nodes["psum"][cur_n].astype(np.uint64)
        nn, pp, ss = [], [], []
        for c in range(8):
            sel = (m >> c) & 1 == 1
            nn.append(ch[sel, c])
            pp.append((cur_p[sel] << np.uint64(3)) | np.uint64(c))
            ss.append((cur_s[sel] + ps[sel, c]) & np.uint64(0xFFFFFFFF))
        cur_n, cur_p, cur_s = np.concatenate(nn), np.concatenate(pp), np.concatenate(ss)
        if lvl + 1 < L:
            cur_n = cur_n & U.IDX if embedded else cur_n
    order = np.argsort(cur_p, kind="stable")
    paths = cur_p[order]
    assert len(paths) < 2 or (paths[1:] > paths[:-1]).all()  # the paths of a DAG are distinct
    return paths, cur_s[order].astype(np.uint32), D.decode(paths)
