"""numpy model of the nearest voxel of arbitrary lattice points (include/mvrt.h, mvrt_svo_nearest_voxels / mvrt_svo_nearest_between / mvrt_svo_transfer_attributes;
DESIGN.md 5.24), written from the definitions of the header alone.  It knows nothing of the descent: for every query the lexicographic minimum of ( d2, vIndex )
over ALL voxels is taken by brute force in int64, in chunks of queries.

  d2(q)    = min over v in B of |q - v|^2, no radius; q is any lattice point, in the grid or not
  near(q)  = the lowest vIndex (rank in ascending Morton code) among the voxels at that distance
  attribs  = colour RGB and emission RGB of voxel near(q), both alpha bytes 255
  limit    d2(q) > maxDist2: dist2 = 2^64 - 1, nearest = 2^32 - 1, attribs 0"""
import numpy as np

from surface_expected import morton

NO_LIMIT = (1 << 64) - 1
NONE = 0xFFFFFFFF


def sorted_set(xyz, attribs=None):
    """-> (xyz (n, 3) int64, attribs (n, 8) uint8) in vIndex order; attribs None = white, no emission"""
    xyz = np.asarray(xyz, np.int64).reshape(-1, 3)
    attribs = np.full((len(xyz), 8), 255, np.uint8) * np.array([1, 1, 1, 1, 0, 0, 0, 1], np.uint8) if attribs is None else np.asarray(attribs, np.uint8).reshape(-1, 8)
    codes = morton(xyz)
    assert len(np.unique(codes)) == len(codes), "the model takes a voxel SET"
    order = np.argsort(codes, kind="stable")
    return xyz[order], attribs[order]


def alpha255(attribs):
    a = np.array(attribs, np.uint8).reshape(-1, 8)
    a[:, 3] = a[:, 7] = 255
    return a


def brute(queries, xyz_sorted, budget=1 << 22):
    """queries (m, 3), xyz_sorted (n, 3) in vIndex order -> (d2 (m,) int64, near (m,) int64).  All arithmetic is int64: a difference is below 2^23, d2 below 2^47.
    argmin returns the first minimum of a row and the voxels stand in vIndex order: the lowest vIndex at the smallest distance"""
    q, v = np.asarray(queries, np.int64).reshape(-1, 3), np.asarray(xyz_sorted, np.int64).reshape(-1, 3)
    d2, near = np.zeros(len(q), np.int64), np.zeros(len(q), np.int64)
    step = max(1, budget // max(1, len(v)))
    for a in range(0, len(q), step):
        d = ((q[a:a + step, None, :] - v[None, :, :]) ** 2).sum(2)
        i = d.argmin(1)
        near[a:a + step], d2[a:a + step] = i, d[np.arange(len(i)), i]
    return d2, near


def nearest_voxels(xyz, attribs, queries, max_dist2=NO_LIMIT):
    """-> {dist2 (m,) uint64, nearest (m,) uint32, attribs (m, 8) uint8} for a set given in any order"""
    xyz, attribs = sorted_set(xyz, attribs)
    d2, near = brute(queries, xyz)
    at = alpha255(attribs[near])
    out_d2, out_near = d2.astype(np.uint64), near.astype(np.uint32)
    if max_dist2 != NO_LIMIT:
        beyond = d2 > int(max_dist2)
        out_d2[beyond], out_near[beyond], at[beyond] = NO_LIMIT, NONE, 0
    return {"dist2": out_d2, "nearest": out_near, "attribs": at}


def nearest_between(a_xyz, b_xyz, offset=(0, 0, 0), max_dist2=NO_LIMIT):
    """every voxel of a, in a's vIndex order, queried as v - offset in b -> the listing and the five numbers of mvrt_svo_nearest_between"""
    a, _ = sorted_set(a_xyz)
    r = nearest_voxels(b_xyz, None, a - np.asarray(offset, np.int64), max_dist2)
    within = r["dist2"] != NO_LIMIT
    far = int(r["dist2"][within].max()) if within.any() else 0
    return {"dist2": r["dist2"], "nearest": r["nearest"], "n": len(a), "maxDist2": far,
            "farthest": int(np.flatnonzero(within & (r["dist2"] == far))[0]) if within.any() else NONE, "zero": int((r["dist2"] == 0).sum()), "beyond": int((~within).sum())}


def transferred(dst_xyz, dst_attribs, src_xyz, src_attribs, offset=(0, 0, 0), max_dist2=NO_LIMIT, flags=3):
    """-> (xyz (n, 3) in dst's vIndex order, the attributes dst ends with, taken (n,) bool = within the limit, changed = the voxels whose 8 bytes differ).  A voxel
    within the limit ends as MVRT_VOXEL_SET stores it: the chosen words from attribs( v - offset ), the other its own, both alpha bytes 255; the rest verbatim"""
    d, da = sorted_set(dst_xyz, dst_attribs)
    r = nearest_voxels(src_xyz, src_attribs, d - np.asarray(offset, np.int64), max_dist2)
    taken = r["dist2"] != NO_LIMIT
    new = da.copy()
    if flags & 1:
        new[taken, 0:4] = r["attribs"][taken, 0:4]
    if flags & 2:
        new[taken, 4:8] = r["attribs"][taken, 4:8]
    new[taken] = alpha255(new[taken])
    return d, new, taken, int((new != da).any(1).sum())
