"""numpy model of mvrt_svo_surface_smooth (include/mvrt.h), written from the rule alone: constrained surface nets on the welded mesh of
surface_expected.py.  Vertex i sits at the lattice corner c_i; its neighbours are the vertices an edge of a listed quad joins it to, one per slot (bit 0 -x,
1 +x, 2 -y, 3 +y, 4 -z, 5 +z).  d starts at 0; one Jacobi iteration, per axis in integers:
    T = sum_j (256 u_ij + d_j) - n d,  delta = rdiv(w T, 256 n),  d <- clamp(d + delta, -limit, limit),  rdiv(a, b) = sign(a) floor((2|a| + b) / (2 b))
and every axis whose d + delta lay outside the box counts as clamped.  Position: q = 256 c + d, t = float32(q) * 2^-8, p = lower + t * dps in fp32.
Vectorised over the vertices; loops over the iterations and the six slots."""
import numpy as np

import surface_expected as S

STEPS = 256
SLOT_OFFSETS = np.array([(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)], np.int64)


def ball(R, r):
    """the cells of [0, R)^3 whose squared distance from ((R - 1) / 2,) * 3 is <= r^2"""
    g = np.argwhere(np.ones((R, R, R), bool))
    return g[((g - (R - 1) / 2.0) ** 2).sum(1) <= r * r]


def rdiv(a, b):
    """nearest, ties away from zero; a int64 array, b > 0 int64 array or scalar"""
    return np.sign(a) * ((2 * np.abs(a) + b) // (2 * b))


def mesh(xyz, res, masks=None):
    """the welded mesh of the set: sorted voxels, masks (given ones are taken without bits 6-7), faces, integer corners of the vertices and indices"""
    xyz = S.sorted_voxels(xyz)
    m = S.masks_of(xyz, res) if masks is None else (np.asarray(masks, np.uint8) & np.uint8(63))
    fv, fd, corners = S.faces(xyz, m)
    r1 = np.uint64(res + 1)
    c = corners.reshape(-1, 3).astype(np.uint64)
    keys = (c[:, 2] * r1 + c[:, 1]) * r1 + c[:, 0]
    uniq, inv = np.unique(keys, return_inverse=True)
    zy = uniq // r1
    grid = np.stack([uniq - zy * r1, zy % r1, zy // r1], -1).astype(np.int64)
    return {"xyz": xyz, "masks": m, "faceVoxel": fv, "faceDir": fd, "corners": grid, "indices": inv.reshape(-1, 4).astype(np.uint32)}


def neighbour_table(corners, indices):
    """-> nbr (m, 6) int64 (-1 where the slot is empty), mask (m,) uint8"""
    m = len(corners)
    nbr = np.full((m, 6), -1, np.int64)
    idx = indices.astype(np.int64)
    for k in range(4):
        for step in (1, 3):
            a, b = idx[:, k], idx[:, (k + step) & 3]
            u = corners[b] - corners[a]
            assert (np.abs(u).sum(1) == 1).all()
            slot = (np.argmax(np.abs(u), 1) * 2 + (u.sum(1) > 0)).astype(np.int64)
            assert ((nbr[a, slot] == -1) | (nbr[a, slot] == b)).all()
            nbr[a, slot] = b
    mask = ((nbr >= 0) << np.arange(6)).sum(1).astype(np.uint8)
    return nbr, mask


def relax(nbr, iterations, weights, limit):
    """-> d (m, 3) int64, clamped"""
    m = len(nbr)
    d = np.zeros((m, 3), np.int64)
    has = nbr >= 0
    n = has.sum(1).astype(np.int64)[:, None]
    unit = (has[:, :, None] * SLOT_OFFSETS[None, :, :]).sum(1)
    clamped = 0
    for k in range(iterations):
        total = np.zeros((m, 3), np.int64)
        for s in range(6):
            total += np.where(has[:, s, None], d[np.maximum(nbr[:, s], 0)], 0)
        T = STEPS * unit + total - n * d
        v = d + rdiv(weights[k & 1] * T, STEPS * n)
        clamped += int((np.abs(v) > limit).sum())
        d = np.clip(v, -limit, limit)
    return d, clamped


def positions(corners, d, lower, dps):
    """q = 256 c + d; t = float32(q) * 2^-8; p = lower + t * dps, multiply and add each rounded to fp32"""
    q = (STEPS * corners + d).astype(np.int32)
    t = q.astype(np.float32) * np.float32(0.00390625)
    return (np.asarray(lower, np.float32) + (t * np.float32(dps)).astype(np.float32)).astype(np.float32)


def smooth(xyz, res, lower, dps, iterations=4, weights=(256, 256), limit=127, masks=None):
    """everything mvrt_svo_surface_smooth returns for the voxel set `xyz` (any order, duplicates allowed)"""
    w = mesh(xyz, res, masks)
    nbr, mask = neighbour_table(w["corners"], w["indices"]) if len(w["corners"]) else (np.zeros((0, 6), np.int64), np.zeros(0, np.uint8))
    d, clamped = relax(nbr, iterations, weights, limit)
    w.update(nbr=nbr, neighbours=mask, displacements=d.astype(np.int32), clamped=clamped, vertices=positions(w["corners"], d, lower, dps))
    return w


def fixed_point(w):
    """the positions in steps of 1/256 cell, (m, 3) int64"""
    return STEPS * w["corners"] + w["displacements"].astype(np.int64)
