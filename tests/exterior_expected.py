"""numpy model of the exterior masks (include/mvrt.h, mvrt_svo_surface_exterior_masks), written from the semantics alone, both ways:

(E1) the plain exposure mask of surface_expected.masks_of with the bits cleared whose neighbour cell is one of the enclosed cells of fill_expected.enclosed;
(E2) the plain exposure mask the same voxel has in fill_expected.filled_set, the set with its enclosed cells added -- where a filled cell itself has no face.

Both take the voxel set in any order and answer in vIndex (Morton) order."""
import numpy as np

import fill_expected as F
import surface_expected as S


def exterior_e1(xyz, res):
    """-> (voxels (n, 3) int64 in vIndex order, plain masks, exterior masks), both (n,) uint8"""
    v = S.sorted_voxels(xyz)
    plain = S.masks_of(v, res).astype(np.uint8)
    enclosed = S.morton(F.enclosed(v, res)["xyz"])
    out = plain.copy()
    for d, (axis, step) in enumerate(S.DIRS):
        p = v.copy()
        p[:, axis] += step
        inside = (p[:, axis] >= 0) & (p[:, axis] < res)
        hidden = np.zeros(len(v), bool)
        hidden[inside] = np.isin(S.morton(p[inside]), enclosed)
        assert not (hidden & ((plain >> d) & 1 == 0)).any()  # an enclosed cell is empty
        out[hidden] &= np.uint8(~(1 << d) & 0xFF)
    return v, plain, out


def exterior_e2(xyz, res):
    """-> (exterior masks (n,) uint8 in vIndex order, masks of the filled cells): the latter must all be 0"""
    v = S.sorted_voxels(xyz)
    f = S.sorted_voxels(F.filled_set(v, res))
    mf = S.masks_of(f, res).astype(np.uint8)
    own = np.isin(S.morton(f), S.morton(v))
    assert own.sum() == len(v)
    return mf[own], mf[~own]


def popcount(masks):
    return int(np.unpackbits(np.asarray(masks, np.uint8)[:, None], axis=1).sum())


def exterior(xyz, res):
    """everything mvrt_svo_surface_exterior_masks returns: {xyz, plain, masks, nFaces, nHidden}"""
    v, plain, ext = exterior_e1(xyz, res)
    return {"xyz": v, "plain": plain, "masks": ext, "nFaces": popcount(ext), "nHidden": popcount(plain) - popcount(ext)}
