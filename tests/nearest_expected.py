"""numpy model of the nearest voxel of the enclosed cells (include/mvrt.h, mvrt_svo_enclosed_nearest / mvrt_svo_fill_enclosed_nearest), written from
the header alone.  No scipy, and none of the three passes of the library: the cells are those of fill_expected.enclosed, and for every cell the minimum over ALL
voxels of the packed ( squared distance << 32 | vIndex ) is taken by brute force, in chunks of cells.

  d2(c)    = min over v in A of |c - v|^2, no radius
  near(c)  = the lowest vIndex (rank in ascending Morton code) among the voxels at that distance
  attribs  = colour RGB and emission RGB of voxel near(c), both alpha bytes 255
The fill: the set with every enclosed cell added, carrying those attributes; near is taken on the set before the fill."""
import numpy as np

import fill_expected
from surface_expected import morton


def _sorted(xyz, attribs):
    xyz = np.asarray(xyz, np.int64).reshape(-1, 3)
    attribs = np.full((len(xyz), 8), 255, np.uint8) * np.array([1, 1, 1, 1, 0, 0, 0, 1], np.uint8) if attribs is None else np.asarray(attribs, np.uint8).reshape(-1, 8)
    codes = morton(xyz)
    assert len(np.unique(codes)) == len(codes), "the model takes a voxel SET"
    order = np.argsort(codes, kind="stable")
    return xyz[order], attribs[order]


def _alpha255(attribs):
    a = np.array(attribs, np.uint8).reshape(-1, 8)
    a[:, 3] = a[:, 7] = 255
    return a


def nearest_of(cells, xyz_sorted, budget=1 << 24):
    """cells (m, 3), xyz_sorted (n, 3) in vIndex order -> (d2 (m,) int64, near (m,) int64) by brute force over all voxels"""
    cells, v = np.asarray(cells, np.int64).reshape(-1, 3), np.asarray(xyz_sorted, np.int64).reshape(-1, 3)
    d2, near = np.zeros(len(cells), np.int64), np.zeros(len(cells), np.int64)
    if len(cells) == 0:
        return d2, near
    # |c - v|^2 = |c|^2 + |v|^2 - 2 c.v for every pair, in float64: all terms are integers below 2^53 (coordinates taken from the voxels' lowest corner), so the
    # sums are exact.  argmin returns the first minimum of a row, and the voxels stand in vIndex order: the lowest vIndex at the smallest distance
    lo = v.min(0)
    c, w = (cells - lo).astype(np.float64), (v - lo).astype(np.float64)
    assert max(np.abs(c).max(), w.max()) < 1 << 24
    w2 = (w * w).sum(1)
    step = max(1, budget // max(1, len(v)))
    for a in range(0, len(cells), step):
        d = (c[a:a + step] ** 2).sum(1)[:, None] + w2[None] - 2.0 * (c[a:a + step] @ w.T)
        i = d.argmin(1)
        near[a:a + step], d2[a:a + step] = i, d[np.arange(len(i)), i].astype(np.int64)
    return d2, near


def enclosed_nearest(xyz, attribs, res):
    """-> {xyz (n, 3) uint32 ascending Morton, region (n,) uint32, dist2 (n,) uint32, nearest (n,) uint32, attribs (n, 8) uint8, nRegions}"""
    xyz, attribs = _sorted(xyz, attribs)
    e = fill_expected.enclosed(xyz, res)
    d2, near = nearest_of(e["xyz"], xyz)
    assert len(d2) == 0 or d2.max() < 1 << 20  # the bound of the header, on the sets the tests use
    return {"xyz": e["xyz"], "region": e["region"], "dist2": d2.astype(np.uint32), "nearest": near.astype(np.uint32), "attribs": _alpha255(attribs[near]).reshape(-1, 8),
            "nRegions": e["nRegions"]}


def filled(xyz, attribs, res):
    """the set after the fill -> (xyz (n, 3) uint32 ascending Morton, attribs (n, 8) uint8): the voxels keep their bytes, every enclosed cell takes the attributes
    of its nearest voxel"""
    xyz, attribs = _sorted(xyz, attribs)
    e = enclosed_nearest(xyz, attribs, res)
    both, at = np.concatenate([xyz, e["xyz"].astype(np.int64)]), np.concatenate([attribs, e["attribs"]])
    order = np.argsort(morton(both), kind="stable")
    return both[order].astype(np.uint32).reshape(-1, 3), at[order].reshape(-1, 8)
