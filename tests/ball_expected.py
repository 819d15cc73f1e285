"""numpy model of the round offsets of a voxel set (include/mvrt.h, mvrt_svo_distance_cells / _depth_voxels / _dilate_ball / _erode_ball / _close_ball / _open_ball;
DESIGN.md 5.21), written from the definitions alone.  No scipy.

Grid [0, R)^3, A the voxel set, rho = radius2 in [1, 1024], B(rho) = the integer offsets o with |o|^2 <= rho.
  outer distance  for an in-grid cell c not in A: d2(c) = min over v in A of |c - v|^2; near(c) = the lowest vIndex among the voxels at that distance
  dilation        D(A) = A + { c in the grid, not in A, d2(c) <= rho }; a new cell takes colour and emission RGB of voxel near(c), both alpha bytes 255
  depth           for v in A: e2(v) = min over IN-GRID cells c not in A of |v - c|^2: outside the grid counts as occupied
  erosion         E(A) = { v in A : e2(v) > rho }; the survivors keep their 8 bytes
  closing         E(D(A)); opening: the set D(E(A)), every voxel of it with its ORIGINAL bytes
Everything is listed in ascending Morton code (x = bit 0 of each group), which is the vIndex order of the octree.

The dense form works on the voxels' box grown by 2 k, k = floor( sqrt( rho ) ) (a closing reaches k beyond the dilated set), and takes the minimum over the offsets
of B(rho) of shifted arrays of the packed ( d2 << 32 | vIndex ).  The sparse form (sparse=True) lists voxel + offset for every pair, for a few voxels at gridRes
2^21 or a large rho."""
import numpy as np

from surface_expected import morton

INF = np.int64(1) << np.int64(62)


def reach(rho):
    k = 0
    while (k + 1) * (k + 1) <= rho:
        k += 1
    return k


def ball_offsets(rho):
    """-> (offsets (m, 3) int64, their squared lengths (m,) int64), the centre included"""
    k = reach(rho)
    r = np.arange(-k, k + 1, dtype=np.int64)
    o = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    d2 = (o * o).sum(1)
    return o[d2 <= rho], d2[d2 <= rho]


def _sorted(xyz, attribs):
    xyz = np.asarray(xyz, np.int64).reshape(-1, 3)
    attribs = np.full((len(xyz), 8), 255, np.uint8) * np.array([1, 1, 1, 1, 0, 0, 0, 1], np.uint8) if attribs is None else np.asarray(attribs, np.uint8).reshape(-1, 8)
    codes = morton(xyz)
    assert len(np.unique(codes)) == len(codes), "the model takes a voxel SET"
    order = np.argsort(codes, kind="stable")
    return xyz[order], attribs[order]


def _by_code(xyz, *arrays):
    order = np.argsort(morton(xyz), kind="stable")
    return (xyz[order],) + tuple(a[order] for a in arrays)


def _alpha255(attribs):
    a = np.array(attribs, np.uint8).reshape(-1, 8)
    a[:, 3] = a[:, 7] = 255
    return a


# ---- the two distances: cells x (d2, payload) --------------------------------------------------------------------------------------------------------------------
def _dense_box(xyz, res, rho):
    grow = 2 * reach(rho)
    lo, hi = np.maximum(xyz.min(0) - grow, 0), np.minimum(xyz.max(0) + grow, res - 1)
    shape = tuple(hi - lo + 1)
    assert np.prod(shape) * len(ball_offsets(rho)[1]) <= 1 << 30, "too large for the dense form"
    return lo, shape


def _dense_min(packed, rho):
    """packed: int64 box, d2 << 32 | payload on the sources and INF elsewhere -> per cell the minimum over o in B(rho) of packed[c + o] + ( |o|^2 << 32 ).  A cell
    beyond the box holds no source."""
    k = reach(rho)
    pad = np.pad(packed, k, constant_values=INF)
    out = np.full(packed.shape, INF, np.int64)
    sx, sy, sz = packed.shape
    for o, d2 in zip(*ball_offsets(rho)):
        s = pad[k + o[0]:k + o[0] + sx, k + o[1]:k + o[1] + sy, k + o[2]:k + o[2] + sz]
        out = np.minimum(out, np.where(s < INF, s + (d2 << np.int64(32)), INF))
    return out


def _outer(xyz, res, rho, sparse):
    """xyz sorted by code -> (cells (m, 3) int64 ascending Morton, d2 (m,), near (m,)): the in-grid cells outside the set with d2 <= rho"""
    if sparse:
        off, od2 = ball_offsets(rho)
        c = (xyz[:, None, :] + off[None]).reshape(-1, 3)
        d2, vi = np.tile(od2, len(xyz)), np.repeat(np.arange(len(xyz), dtype=np.int64), len(off))
        ok = np.all((c >= 0) & (c < res), axis=1)
        c, d2, vi = c[ok], d2[ok], vi[ok]
        codes = morton(c)
        ok = ~np.isin(codes, morton(xyz))
        c, d2, vi, codes = c[ok], d2[ok], vi[ok], codes[ok]
        order = np.lexsort((vi, d2, codes))  # by code, then d2, then vIndex
        c, d2, vi, codes = c[order], d2[order], vi[order], codes[order]
        head = np.ones(len(codes), bool)
        head[1:] = codes[1:] != codes[:-1]
        return c[head], d2[head], vi[head]
    lo, shape = _dense_box(xyz, res, rho)
    packed = np.full(shape, INF, np.int64)
    p = xyz - lo
    packed[p[:, 0], p[:, 1], p[:, 2]] = np.arange(len(xyz), dtype=np.int64)
    best = _dense_min(packed, rho)
    best[p[:, 0], p[:, 1], p[:, 2]] = INF  # (cells of the set are not listed)
    q = np.argwhere(best < INF)
    v = best[q[:, 0], q[:, 1], q[:, 2]]
    return _by_code(q + lo, v >> np.int64(32), v & np.int64(0xFFFFFFFF))


def _depth(xyz, res, rho, sparse):
    """xyz sorted by code -> e2 (n,) int64 per voxel, INF where it is above rho"""
    if sparse:
        off, od2 = ball_offsets(rho)
        c = (xyz[:, None, :] + off[None]).reshape(-1, 3)
        empty = np.all((c >= 0) & (c < res), axis=1) & ~np.isin(morton(np.clip(c, 0, res - 1)), morton(xyz))
        d2 = np.where(empty.reshape(len(xyz), len(off)), od2[None], INF)
        return d2.min(1)
    lo, shape = _dense_box(xyz, res, rho)
    packed = np.zeros(shape, np.int64)  # every cell of the box is in the grid: empty, distance 0, no payload
    p = xyz - lo
    packed[p[:, 0], p[:, 1], p[:, 2]] = INF
    best = _dense_min(packed, rho)
    return np.where(best[p[:, 0], p[:, 1], p[:, 2]] < INF, best[p[:, 0], p[:, 1], p[:, 2]] >> np.int64(32), INF)


# ---- the calls -----------------------------------------------------------------------------------------------------------------------------------------------
def distance_cells(xyz, attribs, res, rho, sparse=False):
    """-> {xyz (n, 3) uint32 ascending Morton, dist2 (n,) uint32, nearest (n,) uint32, attribs (n, 8) uint8}: the cells of D(A) \\ A"""
    xyz, attribs = _sorted(xyz, attribs)
    c, d2, near = _outer(xyz, res, rho, sparse)
    return {"xyz": c.astype(np.uint32).reshape(-1, 3), "dist2": d2.astype(np.uint32), "nearest": near.astype(np.uint32), "attribs": _alpha255(attribs[near])}


def depth_voxels(xyz, res, rho, sparse=False):
    """-> {vIndex (n,) uint32 ascending, depth2 (n,) uint32}: the voxels with e2 <= rho"""
    xyz, _ = _sorted(xyz, None)
    e2 = _depth(xyz, res, rho, sparse)
    shallow = np.flatnonzero(e2 < INF)
    return {"vIndex": shallow.astype(np.uint32), "depth2": e2[shallow].astype(np.uint32)}


def _dilated(xyz, attribs, res, rho, sparse):
    c, _, near = _outer(xyz, res, rho, sparse)
    return _by_code(np.concatenate([xyz, c]), np.concatenate([attribs, _alpha255(attribs[near])]))


def _eroded(xyz, attribs, res, rho, sparse):
    if len(xyz) == 0:
        return xyz, attribs
    keep = _depth(xyz, res, rho, sparse) == INF
    return xyz[keep], attribs[keep]


def ball(op, xyz, attribs, res, rho, sparse=False):
    """op in dilate / erode / close / open -> (xyz (n, 3) uint32 ascending Morton, attribs (n, 8) uint8).  An erosion may leave nothing: the calls refuse that,
    the model returns the empty set."""
    xyz, attribs = _sorted(xyz, attribs)
    out, at = xyz, attribs
    for half in {"dilate": "d", "erode": "e", "close": "de", "open": "ed"}[op]:
        if len(out):
            out, at = (_dilated if half == "d" else _eroded)(out, at, res, rho, sparse)
    if op == "open" and len(out):  # a pure removal: the original bytes
        index = {int(c): i for i, c in enumerate(morton(xyz))}
        at = attribs[[index[int(c)] for c in morton(out)]]
    return out.astype(np.uint32).reshape(-1, 3), at.reshape(-1, 8)
