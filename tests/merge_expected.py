"""numpy model of the merged surface (include/mvrt.h, mvrt_svo_surface_merged), written from the rule alone.

Faces are those of surface_expected.  A face of direction d with normal axis a lies in plane p = the voxel's coordinate on a and has the in-plane coordinates
(u, v) = the voxel's coordinates on the two other axes, the lower-numbered one u.  Mergeable: same d, same p, equal attribute entries (8 bytes; any with
ANY_ATTRIBUTE).  Step 1: within (d, p, v) maximal runs at consecutive u, each face mergeable with the one before.  Step 2: among runs with equal
(d, p, u0, du) and attribute, maximal sequences at consecutive v.  Order: ascending (d, p, u0, v0).  Corners: anchor voxel + corner offset scaled by du on
u, dv on v, 1 on the normal axis; positions and weld as in surface_expected."""
import numpy as np

import surface_expected as S

ANY_ATTRIBUTE, WELD = 1, 2
UV_AXES = {0: (1, 2), 1: (0, 2), 2: (0, 1)}  # normal axis -> (u axis, v axis)


def _chains(fields, step, same):
    """rows sorted by `fields` (most significant first) then by `step`: head flags of the maximal chains where `fields` and `same` repeat and `step` grows by 1"""
    head = np.ones(len(step), bool)
    link = step[1:] == step[:-1] + 1
    for f in list(fields) + list(same):
        link &= f[1:] == f[:-1]
    head[1:] = ~link
    return head


def merged(xyz, attrs, res, lower, dps, flags=0):
    """xyz: the voxel set in vIndex order (surface_expected.sorted_voxels); attrs: (n, 8) uint8 in the same order, or None = all equal.
    -> dict of nFaces, rectVoxel, rectDir, rectSize (n, 2), corners (n, 4, 3) int64, positions (n, 4, 3); with WELD also vertices, indices"""
    xyz = np.asarray(xyz, np.int64).reshape(-1, 3)
    assert np.all(np.diff(S.morton(xyz).astype(np.int64)) > 0), "vIndex order expected"
    masks = S.masks_of(xyz, res)
    if attrs is None or flags & ANY_ATTRIBUTE:
        a64 = np.zeros(len(xyz), np.uint64)
    else:
        a64 = np.ascontiguousarray(attrs, np.uint8).reshape(-1, 8).view(np.uint64).reshape(-1)
    out = {k: [] for k in ("rectVoxel", "rectDir", "rectSize", "corners")}
    for d, (axis, _) in enumerate(S.DIRS):
        ua, va = UV_AXES[axis]
        vox = np.nonzero((masks >> d) & 1)[0]
        if len(vox) == 0:
            continue
        p, u, v, at = xyz[vox, axis], xyz[vox, ua], xyz[vox, va], a64[vox]
        o = np.lexsort((u, v, p))  # rows
        vox, p, u, v, at = vox[o], p[o], u[o], v[o], at[o]
        start = np.nonzero(_chains((p, v), u, (at,)))[0]
        du = np.diff(np.append(start, len(vox)))
        vox, p, u0, v, at = vox[start], p[start], u[start], v[start], at[start]
        o = np.lexsort((v, u0, p))  # stacks
        vox, p, u0, v, at, du = vox[o], p[o], u0[o], v[o], at[o], du[o]
        start = np.nonzero(_chains((p, u0), v, (du, at)))[0]
        dv = np.diff(np.append(start, len(vox)))
        vox, du = vox[start], du[start]  # already ascending (p, u0, v0)
        scale = np.ones((len(vox), 3), np.int64)
        scale[:, ua], scale[:, va] = du, dv
        out["rectVoxel"].append(vox.astype(np.uint32))
        out["rectDir"].append(np.full(len(vox), d, np.uint8))
        out["rectSize"].append(np.stack([du, dv], -1).astype(np.uint32))
        out["corners"].append(xyz[vox][:, None, :] + S.CORNER_OFFSETS[S.FACE_CORNERS[d]][None] * scale[:, None, :])
    empty = {"rectVoxel": np.zeros(0, np.uint32), "rectDir": np.zeros(0, np.uint8), "rectSize": np.zeros((0, 2), np.uint32), "corners": np.zeros((0, 4, 3), np.int64)}
    out = {k: (np.concatenate(v) if v else empty[k]) for k, v in out.items()}
    out["nFaces"] = int(sum(bin(m).count("1") for m in masks.tolist()))
    out["positions"] = S.positions(out["corners"], lower, dps)
    if flags & WELD:
        out["vertices"], out["indices"] = S.weld(out["corners"], res, lower, dps)
    return out


def rasterise(xyz, rectVoxel, rectDir, rectSize):
    """the faces the rectangles cover, as rows (x, y, z, d), one per face, in rectangle order"""
    xyz = np.asarray(xyz, np.int64)
    rows = []
    for vox, d, (du, dv) in zip(rectVoxel.tolist(), rectDir.tolist(), np.asarray(rectSize).tolist()):
        ua, va = UV_AXES[S.DIRS[d][0]]
        j, i = np.meshgrid(np.arange(dv), np.arange(du), indexing="ij")
        r = np.empty((du * dv, 4), np.int64)
        r[:, :3], r[:, 3] = xyz[vox], d
        r[:, ua] += i.reshape(-1)
        r[:, va] += j.reshape(-1)
        rows.append(r)
    return np.concatenate(rows) if rows else np.zeros((0, 4), np.int64)


def face_rows(xyz, masks):
    """the faces of surface_expected.faces as rows (x, y, z, d)"""
    fv, fd, _ = S.faces(np.asarray(xyz, np.int64), masks)
    return np.concatenate([np.asarray(xyz, np.int64)[fv], fd[:, None].astype(np.int64)], 1)


def same_face_set(rows_a, rows_b):
    """both are the same set and neither names a face twice"""
    a, b = np.unique(rows_a, axis=0), np.unique(rows_b, axis=0)
    return len(a) == len(rows_a) and len(b) == len(rows_b) and np.array_equal(a, b)
