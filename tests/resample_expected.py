"""numpy int64 model of the affine resampling of a voxel set (include/mvrt.h, mvrt_svo_resample_voxels / mvrt_svo_resample), written from the
semantics alone.

S = the voxels of the source on [0, Rs)^3, F = 24.  A destination cell c of [0, Rd)^3 belongs to the result when s = floor( ( m (2c + 1) + t ) / 2^(F+1) ), taken in
int64, lies in [0, Rs)^3 and is a voxel of S; it takes that voxel's colour and emission RGB with both alpha bytes 255, and source(c) is the voxel's vIndex.  Order:
ascending Morton code in the destination grid.  Two forms: `dense` evaluates the rule on every cell (Rd <= 128), `sparse` refines the destination grid top-down with a
conservative integer bounding box per node and is what large grids are checked against; the CPU tests compare the two."""
import itertools

import numpy as np

from surface_expected import decode, morton

F = 24
ONE = 1 << F  # 1.0 in m
HALF = 1 << F  # 0.5 in t (t is Q25)
M_MAX, T_MAX = 1 << 30, 1 << 52


def transform_ok(m, t):
    return all(abs(int(v)) <= M_MAX for v in np.asarray(m, object).reshape(9)) and all(abs(int(v)) <= T_MAX for v in np.asarray(t, object).reshape(3))


def from_cells(A, b=(0.0, 0.0, 0.0)):
    """s = A c + b in cell coordinates -> (m (9,) int64, t (3,) int64), rounded to nearest"""
    A, b = np.asarray(A, np.float64).reshape(9), np.asarray(b, np.float64).reshape(3)
    return np.rint(A * 2.0 ** F).astype(np.int64), np.rint(b * 2.0 ** (F + 1)).astype(np.int64)


def identity():
    return np.array([ONE, 0, 0, 0, ONE, 0, 0, 0, ONE], np.int64), np.zeros(3, np.int64)


def signed_permutation(perm, flips, res):
    """source axis i reads destination axis perm[i], mirrored about the centre of a grid of `res` cells where flips[i]: s_i = c_perm[i] or res - 1 - c_perm[i], exact"""
    m, t = np.zeros(9, np.int64), np.zeros(3, np.int64)
    for i in range(3):
        m[3 * i + perm[i]] = -ONE if flips[i] else ONE
        t[i] = res * 2 * ONE if flips[i] else 0
    return m, t


def all_signed_permutations(res):
    return [(p, f, signed_permutation(p, f, res)) for p in itertools.permutations(range(3)) for f in itertools.product((0, 1), repeat=3)]


def about_centre(A, src_res, dst_res, shift=(0.0, 0.0, 0.0)):
    """the map s = A ( c - centre of the destination grid ) + centre of the source grid + shift, in cell coordinates (points, a cell centre is c + 0.5)"""
    A = np.asarray(A, np.float64).reshape(3, 3)
    b = np.full(3, src_res / 2.0) - A @ np.full(3, dst_res / 2.0) + np.asarray(shift, np.float64)
    return from_cells(A, b)


def rotation(axis, degrees):
    """Rodrigues: the 3x3 rotation by `degrees` about `axis`"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    r = np.radians(degrees)
    return np.eye(3) + np.sin(r) * K + (1 - np.cos(r)) * (K @ K)


def point(m, t, c):
    """the point rule: destination cells c (n, 3) -> source cells s (n, 3) int64, inside or not"""
    c = np.asarray(c, np.int64).reshape(-1, 3)
    M, t = np.asarray(m, np.int64).reshape(3, 3), np.asarray(t, np.int64).reshape(3)
    return ((2 * c + 1) @ M.T + t) >> (F + 1)  # (>> of a negative int64 is the floor)


def _source(src_xyz, src_attribs):
    src_xyz = np.asarray(src_xyz, np.int64).reshape(-1, 3)
    codes = morton(src_xyz)
    order = np.argsort(codes, kind="stable")
    assert len(np.unique(codes)) == len(codes)
    at = np.asarray(src_attribs, np.uint8).reshape(-1, 8)[order].copy()
    at[:, 3] = 255
    at[:, 7] = 255
    return codes[order], at


def _lookup(codes, at, s, src_res, cells):
    """of the destination cells `cells` with source cells s: the result among them, in the order given"""
    inside = ((s >= 0) & (s < src_res)).all(1)
    sc = morton(s[inside])
    i = np.searchsorted(codes, sc)
    hit = (i < len(codes)) & (codes[np.minimum(i, max(len(codes) - 1, 0))] == sc) if len(codes) else np.zeros(len(sc), bool)
    return cells[inside][hit], at[i[hit]], i[hit].astype(np.uint32)


def _result(xyz, at, src):
    order = np.argsort(morton(xyz), kind="stable")
    return {"xyz": xyz[order].astype(np.uint32).reshape(-1, 3), "attribs": at[order].reshape(-1, 8), "source": src[order].astype(np.uint32)}


def dense(src_xyz, src_attribs, src_res, m, t, dst_res):
    """every cell of the destination grid through the point rule -> {xyz (n, 3) uint32, attribs (n, 8) uint8, source (n,) uint32}"""
    assert dst_res <= 128
    codes, at = _source(src_xyz, src_attribs)
    cells = np.stack(np.meshgrid(*[np.arange(dst_res, dtype=np.int64)] * 3, indexing="ij"), -1).reshape(-1, 3)
    return _result(*_lookup(codes, at, point(m, t, cells), src_res, cells))


def node_box(m, t, c0, k, src_res):
    """nodes of 2^k cells per axis with lowest cells c0 (n, 3): the exact bounding box of the source cells of their sample points, clipped to the source grid ->
    (lo (n, 3), hi (n, 3), hits (n,) bool = the box meets the grid)"""
    c0 = np.asarray(c0, np.int64).reshape(-1, 3)
    M, t = np.asarray(m, np.int64).reshape(3, 3), np.asarray(t, np.int64).reshape(3)
    q_lo, q_hi = 2 * c0 + 1, 2 * (c0 + (1 << k)) - 1
    a, b = q_lo[:, None, :] * M[None], q_hi[:, None, :] * M[None]  # (n, i, j)
    s_min = (np.minimum(a, b).sum(2) + t) >> (F + 1)
    s_max = (np.maximum(a, b).sum(2) + t) >> (F + 1)
    hits = ((s_max >= 0) & (s_min < src_res)).all(1)
    return np.clip(s_min, 0, src_res - 1), np.clip(s_max, 0, src_res - 1), hits


def sparse(src_xyz, src_attribs, src_res, m, t, dst_res, stats=None):
    """the same result by refining the destination grid top-down: a node is kept when the box of its sample points, widened to whole coarse cells of the source at the
    smallest level where it spans at most two per axis, holds a voxel.  stats (a list): the frontier sizes per level are appended"""
    codes, at = _source(src_xyz, src_attribs)
    levels = int(dst_res).bit_length() - 1
    assert 1 << levels == dst_res
    occupied = {}  # h -> the sorted coarse codes of the source at shift h

    def occ(h):
        if h not in occupied:
            occupied[h] = np.unique(codes >> np.uint64(3 * h))
        return occupied[h]

    frontier = np.zeros(1, np.uint64)
    for l in range(1, levels):
        k = levels - l
        child = ((frontier[:, None] << np.uint64(3)) | np.arange(8, dtype=np.uint64)[None]).reshape(-1)
        lo, hi, keep = node_box(m, t, decode(child) << k, k, src_res)
        h = np.zeros(len(child), np.int64)
        for _ in range(22):
            wide = keep & (((hi >> h[:, None]) - (lo >> h[:, None])).max(1) > 1)
            if not wide.any():
                break
            h[wide] += 1
        found = np.zeros(len(child), bool)
        for hv in np.unique(h[keep]):
            sel = np.flatnonzero(keep & (h == hv))
            for d in itertools.product((0, 1), repeat=3):
                cc = np.minimum((lo[sel] >> hv) + np.array(d), hi[sel] >> hv)
                found[sel] |= np.isin(morton(cc), occ(int(hv)))
        frontier = child[found]
        if stats is not None:
            stats.append(len(frontier))
        if len(frontier) == 0:
            break
    if levels == 1 or len(frontier):
        child = ((frontier[:, None] << np.uint64(3)) | np.arange(8, dtype=np.uint64)[None]).reshape(-1)
        cells = decode(child)
        out = _result(*_lookup(codes, at, point(m, t, cells), src_res, cells))
    else:
        out = _result(np.zeros((0, 3), np.int64), np.zeros((0, 8), np.uint8), np.zeros(0, np.uint32))
    if stats is not None and (levels == 1 or len(frontier)):
        stats.append(len(out["xyz"]))
    return out


def from_world(world, src_lower, src_dps, dst_lower, dst_dps):
    """mvrt_cell_transform_from_world in numpy float64: world 3x4 row-major, p_dst = W p_src + w -> (m (9,) int64, t (3,) int64) before any range check, as floats
    rounded to nearest"""
    w = np.asarray(world, np.float64).reshape(3, 4)
    inv = np.linalg.inv(w[:, :3])
    sl, dl = np.asarray(src_lower, np.float32).astype(np.float64), np.asarray(dst_lower, np.float32).astype(np.float64)
    sd, dd = float(np.float32(src_dps)), float(np.float32(dst_dps))
    A = inv * (dd / sd)
    b = (inv @ (dl - w[:, 3]) - sl) / sd
    return A.reshape(9) * 2.0 ** F, b * 2.0 ** (F + 1)
