"""numpy model of the boolean operations between two voxel sets (include/mvrt.h, mvrt_svo_combine_voxels / mvrt_svo_combine), written from the
semantics alone.

A = the voxels of a on the grid [0, R)^3; B' = { v + o : v in B, v + o in [0, R)^3 }, the sum in int64; clipped = |B| - |B'|.  UNION = A + B', INTERSECTION =
A n B', DIFFERENCE = A \\ B', XOR = (A \\ B') + (B' \\ A), in ascending Morton code of a's grid.  A result voxel that is in A keeps a's 8 bytes; one of B' alone takes
b's colour and emission RGB with both alpha bytes 255; under ATTRIB_B the overlap, where it survives (UNION, INTERSECTION), takes b's bytes by the same rule.
source = 1 (A only), 2 (B' only), 3 (both)."""
import numpy as np

from surface_expected import decode, morton

UNION, INTERSECTION, DIFFERENCE, XOR = 0, 1, 2, 3
OPS = (UNION, INTERSECTION, DIFFERENCE, XOR)
ATTRIB_B = 1
SET, REMOVE = 1, 0


def _sorted(xyz, attribs):
    """a voxel list (distinct cells) in ascending Morton code: codes, (n, 8) uint8 attributes"""
    xyz = np.asarray(xyz, np.int64).reshape(-1, 3)
    attribs = np.asarray(attribs, np.uint8).reshape(-1, 8)
    codes = morton(xyz)
    order = np.argsort(codes, kind="stable")
    assert len(np.unique(codes)) == len(codes)
    return codes[order], attribs[order]


def translate(b_xyz, b_attribs, res, offset=None):
    """B' -> (codes ascending, attributes with both alpha bytes 255, clipped)"""
    b_xyz = np.asarray(b_xyz, np.int64).reshape(-1, 3)
    b_attribs = np.asarray(b_attribs, np.uint8).reshape(-1, 8).copy()
    moved = b_xyz + (np.zeros(3, np.int64) if offset is None else np.asarray(offset, np.int64).reshape(3))
    inside = ((moved >= 0) & (moved < res)).all(1)
    b_attribs[:, 3] = 255
    b_attribs[:, 7] = 255
    codes, at = _sorted(moved[inside], b_attribs[inside])
    return codes, at, int(len(b_xyz) - inside.sum())


def combine(a_xyz, a_attribs, b_xyz, b_attribs, res, op, offset=None, flags=0):
    """-> {xyz (n, 3) uint32, attribs (n, 8) uint8, source (n,) uint8, overlap, clipped}"""
    ca, aa = _sorted(a_xyz, a_attribs)
    cb, ab, clipped = translate(b_xyz, b_attribs, res, offset)
    a_in_b, b_in_a = np.isin(ca, cb), np.isin(cb, ca)
    if op == UNION:
        codes = np.union1d(ca, cb)
    elif op == INTERSECTION:
        codes = ca[a_in_b]
    elif op == DIFFERENCE:
        codes = ca[~a_in_b]
    elif op == XOR:
        codes = np.union1d(ca[~a_in_b], cb[~b_in_a])
    else:
        raise ValueError(op)
    in_a, in_b = np.isin(codes, ca), np.isin(codes, cb)
    attribs = np.zeros((len(codes), 8), np.uint8)
    attribs[in_a] = aa[np.searchsorted(ca, codes[in_a])]
    from_b = in_b & ~in_a if not (flags & ATTRIB_B) else in_b
    attribs[from_b] = ab[np.searchsorted(cb, codes[from_b])]
    source = (in_a.astype(np.uint8) | (in_b.astype(np.uint8) << 1)).astype(np.uint8)
    return {"xyz": decode(codes).astype(np.uint32), "attribs": attribs, "source": source, "overlap": int(a_in_b.sum()), "clipped": clipped}


def edit_lists(a_xyz, a_attribs, b_xyz, b_attribs, res, op, offset=None, flags=0):
    """the batch mvrt_svo_edit_voxels stands for: (xyz (m, 3) uint32, attribs (m, 8) uint8, ops (m,) uint8) -- B' \\ A as SET where the operator takes it, the
    overlap as SET under ATTRIB_B where it survives, the voxels of A the operator drops as REMOVE -- and (added, removed)"""
    ca, _ = _sorted(a_xyz, a_attribs)
    cb, ab, _ = translate(b_xyz, b_attribs, res, offset)
    a_in_b, b_in_a = np.isin(ca, cb), np.isin(cb, ca)
    sets = np.zeros(len(cb), bool)
    if op in (UNION, XOR):
        sets |= ~b_in_a
    if (flags & ATTRIB_B) and op in (UNION, INTERSECTION):
        sets |= b_in_a
    drops = {UNION: np.zeros(len(ca), bool), INTERSECTION: ~a_in_b, DIFFERENCE: a_in_b, XOR: a_in_b}[op]
    xyz = np.concatenate([decode(cb[sets]), decode(ca[drops])]).astype(np.uint32)
    attribs = np.concatenate([ab[sets], np.zeros((int(drops.sum()), 8), np.uint8)])
    ops = np.concatenate([np.full(int(sets.sum()), SET, np.uint8), np.full(int(drops.sum()), REMOVE, np.uint8)])
    added = int((~b_in_a).sum()) if op in (UNION, XOR) else 0
    return xyz, attribs, ops, (added, int(drops.sum()))
