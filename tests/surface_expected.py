"""numpy model of the surface extraction (include/mvrt.h, mvrt_svo_surface_*), written from the semantics alone.

Exposure mask: per voxel in vIndex (Morton) order one byte, bit b set when the neighbour in direction b holds no voxel; directions in the
reference's emission order 0 = -Y, 1 = +Y, 2 = -Z, 3 = +X, 4 = +Z, 5 = -X; outside [0, gridRes) is empty.  Faces by vIndex then direction.
Corner c of a voxel at CORNER_OFFSETS[c]; face d has the corners FACE_CORNERS[d].  A corner coordinate c lies at lower + float32(c) * dps,
multiply and add each rounded to fp32.  Weld: key = (cz * (R + 1) + cy) * (R + 1) + cx, vertices = the distinct keys ascending,
indices = ranks: exactly np.unique(keys, return_inverse=True)."""
import numpy as np

DIRS = ((1, -1), (1, +1), (2, -1), (0, +1), (2, +1), (0, -1))  # (axis, step) per direction
CORNER_OFFSETS = np.array([(0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1), (0, 1, 0), (1, 1, 0), (1, 1, 1), (0, 1, 1)], np.int64)
FACE_CORNERS = np.array([(3, 2, 1, 0), (4, 5, 6, 7), (0, 1, 5, 4), (1, 2, 6, 5), (2, 3, 7, 6), (3, 0, 4, 7)], np.int64)


def morton(xyz):
    """(n, 3) -> uint64 codes, x = bit 0, 21 bits per axis"""
    xyz = np.asarray(xyz, np.uint64).reshape(-1, 3)
    m = np.zeros(len(xyz), np.uint64)
    for b in range(21):
        for axis in range(3):
            m |= ((xyz[:, axis] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + axis)
    return m


def decode(m):
    """uint64 codes -> (n, 3) int64"""
    m = np.asarray(m, np.uint64)
    out = np.zeros((len(m), 3), np.int64)
    for b in range(21):
        for axis in range(3):
            out[:, axis] |= (((m >> np.uint64(3 * b + axis)) & np.uint64(1)) << np.uint64(b)).astype(np.int64)
    return out


def sorted_voxels(xyz):
    """the voxel set in vIndex order: distinct coordinates sorted by Morton code, (n, 3) int64"""
    xyz = np.asarray(xyz, np.int64).reshape(-1, 3)
    _, first = np.unique(morton(xyz), return_index=True)
    return xyz[first]


def masks_dense(xyz, res):
    """dense padded boolean grid (gridRes <= 256)"""
    assert res <= 256
    g = np.zeros((res + 2,) * 3, bool)
    g[xyz[:, 0] + 1, xyz[:, 1] + 1, xyz[:, 2] + 1] = True
    out = np.zeros(len(xyz), np.uint8)
    for d, (axis, step) in enumerate(DIRS):
        p = xyz + 1
        p[:, axis] += step
        out |= (~g[p[:, 0], p[:, 1], p[:, 2]]).astype(np.uint8) << d
    return out


def masks_sparse(xyz, res):
    """np.isin on the codes of the shifted coordinates (any gridRes up to 2^21); a neighbour outside the grid is empty without being encoded"""
    codes = morton(xyz)
    out = np.zeros(len(xyz), np.uint8)
    for d, (axis, step) in enumerate(DIRS):
        p = xyz.copy()
        p[:, axis] += step
        inside = (p[:, axis] >= 0) & (p[:, axis] < res)
        present = np.zeros(len(xyz), bool)
        present[inside] = np.isin(morton(p[inside]), codes)
        out |= (~present).astype(np.uint8) << d
    return out


def masks_of(xyz, res):
    return masks_dense(xyz, res) if res <= 256 else masks_sparse(xyz, res)


def faces(xyz, masks):
    """-> faceVoxel (n,) uint32, faceDir (n,) uint8, corner grid coordinates (n, 4, 3) int64"""
    bits = (masks[:, None] >> np.arange(6, dtype=np.uint8)[None, :]) & 1
    v, d = np.nonzero(bits)  # row-major: by voxel, then by direction
    corners = xyz[v][:, None, :] + CORNER_OFFSETS[FACE_CORNERS[d]]
    return v.astype(np.uint32), d.astype(np.uint8), corners.reshape(-1, 4, 3)


def positions(corners, lower, dps):
    """lower + (float)c * dps: one fp32 multiply, one fp32 add"""
    prod = corners.astype(np.float32) * np.float32(dps)
    return (np.asarray(lower, np.float32) + prod).astype(np.float32)


def weld(corners, res, lower, dps):
    """-> vertices (m, 3) float32, indices (n, 4) uint32"""
    r1 = np.uint64(res + 1)
    c = corners.reshape(-1, 3).astype(np.uint64)
    keys = (c[:, 2] * r1 + c[:, 1]) * r1 + c[:, 0]
    uniq, inv = np.unique(keys, return_inverse=True)
    zy = uniq // r1
    grid = np.stack([uniq - zy * r1, zy % r1, zy // r1], -1).astype(np.int64)
    return positions(grid, lower, dps), inv.reshape(-1, 4).astype(np.uint32)


def surface(xyz, res, lower, dps):
    """everything the three calls return for the voxel set `xyz` (any order, duplicates allowed)"""
    xyz = sorted_voxels(xyz)
    m = masks_of(xyz, res)
    fv, fd, corners = faces(xyz, m)
    vertices, indices = weld(corners, res, lower, dps)
    return {"xyz": xyz, "masks": m, "nFaces": int(len(fv)), "faceVoxel": fv, "faceDir": fd, "positions": positions(corners, lower, dps), "vertices": vertices,
            "indices": indices}


def read_ply_quads(path):
    """minimal reader of what apps/scene_io.hpp writePlyQuads writes -> vertices (m, 3) float32, indices (n, 4) uint32, colours (n, 3) uint8"""
    d = open(path, "rb").read()
    end = d.index(b"end_header\n") + len(b"end_header\n")
    head = d[:end].decode().split("\n")
    assert head[0] == "ply" and head[1] == "format binary_little_endian 1.0"
    elements = [h.split() for h in head if h.startswith("element")]
    assert [e[1] for e in elements] == ["vertex", "face"]
    nv, nf = int(elements[0][2]), int(elements[1][2])
    props = [h for h in head if h.startswith("property")]
    assert props == ["property float x", "property float y", "property float z", "property list uchar uint vertex_indices", "property uchar red", "property uchar green",
                     "property uchar blue"]
    vertices = np.frombuffer(d, "<f4", nv * 3, end).reshape(nv, 3)
    rec = np.frombuffer(d, np.uint8, nf * 20, end + nv * 12).reshape(nf, 20)
    assert len(d) == end + nv * 12 + nf * 20 and (rec[:, 0] == 4).all()
    return vertices, np.ascontiguousarray(rec[:, 1:17]).view("<u4").reshape(nf, 4), rec[:, 17:20].copy()
