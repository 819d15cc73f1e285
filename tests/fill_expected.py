"""numpy model of the enclosed-cell classification (include/mvrt.h, mvrt_svo_enclosed_cells / mvrt_svo_fill_enclosed), written from the semantics
alone: a dense grid (cropped to the box the voxels occupy) and an iterative 6-neighbour propagation from the border cells.  No scipy.

An empty cell is exterior when a path of face-neighbouring empty cells joins it to a cell with a coordinate equal to 0 or gridRes - 1; every other empty cell is
enclosed, and its connected component is a region.  The enclosed cells are listed in ascending Morton code (x = bit 0 of each group) and the regions numbered
0, 1, ... by first appearance in that list."""
import numpy as np

from surface_expected import decode, morton


def _grow(seed, empty):
    """the cells of `empty` reachable from `seed` through face neighbours (both (R, R, R) bool, indexed [x, y, z])"""
    reach = seed & empty
    while True:
        n = reach.copy()
        for axis in range(3):
            lo, hi = [slice(None)] * 3, [slice(None)] * 3
            lo[axis], hi[axis] = slice(0, -1), slice(1, None)
            lo, hi = tuple(lo), tuple(hi)
            n[hi] |= reach[lo]
            n[lo] |= reach[hi]
        n &= empty
        if n.sum() == reach.sum():
            return reach
        reach = n


def _box(xyz, res):
    """The bounding box of the voxels grown by one cell on every side, clipped to the grid: -> (lo, empty) with empty (sx, sy, sz) bool indexed [x, y, z].
    Every cell outside the voxels' bounding box is exterior (a straight walk away from the box meets no voxel up to the border), so the classification of the
    box alone, with all six of its faces as seeds, is the classification of the grid: a face of the box is either such a margin or the grid border itself."""
    xyz = np.asarray(xyz, np.int64).reshape(-1, 3)
    lo = np.maximum(xyz.min(0) - 1, 0)
    hi = np.minimum(xyz.max(0) + 1, res - 1)
    assert (hi - lo).max() < 512 and np.prod(hi - lo + 1) <= 1 << 24
    empty = np.ones(tuple(hi - lo + 1), bool)
    p = xyz - lo
    empty[p[:, 0], p[:, 1], p[:, 2]] = False
    return lo, empty


def enclosed_grid(xyz, res):
    """-> (lo, inside): the enclosed empty cells as a bool array over the box at `lo` (see _box)"""
    lo, empty = _box(xyz, res)
    seeds = np.zeros_like(empty)
    for axis in range(3):
        for side in (0, -1):
            s = [slice(None)] * 3
            s[axis] = side
            seeds[tuple(s)] = True
    return lo, empty & ~_grow(seeds, empty)


def enclosed(xyz, res):
    """-> {xyz (n, 3) uint32 in ascending Morton order, region (n,) uint32 by first appearance, nRegions}"""
    lo, inside = enclosed_grid(xyz, res)
    q = np.argwhere(inside)
    q = q[np.argsort(morton(q + lo), kind="stable")]
    region = np.full(len(q), -1, np.int64)
    index = np.full(inside.shape, -1, np.int64)
    index[q[:, 0], q[:, 1], q[:, 2]] = np.arange(len(q))
    n_regions = 0
    for i in range(len(q)):
        if region[i] >= 0:
            continue
        seed = np.zeros_like(inside)
        seed[tuple(q[i])] = True
        region[index[_grow(seed, inside)]] = n_regions
        n_regions += 1
    return {"xyz": (q + lo).astype(np.uint32).reshape(-1, 3), "region": region.astype(np.uint32), "nRegions": n_regions}


def filled_set(xyz, res):
    """the voxel set with its enclosed cells added, (n, 3) int64 in Morton order"""
    xyz = np.asarray(xyz, np.int64).reshape(-1, 3)
    cells = enclosed(xyz, res)["xyz"].astype(np.int64)
    both = np.concatenate([xyz, cells])
    _, first = np.unique(morton(both), return_index=True)
    return both[first]


