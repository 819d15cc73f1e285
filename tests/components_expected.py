"""Model of the connected components of a voxel set (include/mvrt.h, mvrt_svo_components / mvrt_svo_keep_components), written from the definitions
alone: a plain union-find over the voxels in vIndex order.  No scipy.

Grid [0, R)^3, A the voxel set, element FACES (6-connected) or CUBE (26-connected).  Two voxels are adjacent when one is a neighbour of the other inside the grid
(nothing wraps); a component is a class of the transitive closure.  Components are numbered in order of first appearance in ascending Morton code; per component
size, first (the lowest vIndex) and box (min x, y, z, max x, y, z, inclusive).  keep(): component c stays when size(c) >= min_voxels and (keep_largest == 0 or
its rank by (size descending, label ascending) is below keep_largest).

The neighbour of a voxel is looked up among the sorted codes with searchsorted; with sparse=True in a dict keyed by the coordinates, Python integers throughout
(a handful of voxels at gridRes 2^21).  Neither form allocates the grid."""
import numpy as np

from morph_expected import CUBE, FACES, OFFSETS, _sorted
from surface_expected import morton

__all__ = ["FACES", "CUBE", "components", "keep", "dropped"]


def _pairs_searchsorted(xyz, res, element):
    codes = morton(xyz)
    out = []
    for d in OFFSETS[element]:
        p = xyz + np.array(d, np.int64)
        inside = np.flatnonzero(((p >= 0) & (p < res)).all(1))
        c = morton(p[inside])
        k = np.minimum(np.searchsorted(codes, c), len(codes) - 1)
        hit = codes[k] == c
        out.append(np.stack([inside[hit], k[hit]], 1))
    return np.concatenate(out)


def _pairs_sparse(xyz, res, element):
    index = {tuple(int(v) for v in p): i for i, p in enumerate(xyz)}
    out = []
    for (x, y, z), i in index.items():
        for dx, dy, dz in OFFSETS[element]:
            q = (x + dx, y + dy, z + dz)
            if min(q) >= 0 and max(q) < res and q in index:
                out.append((i, index[q]))
    return np.array(out, np.int64).reshape(-1, 2)


def components(xyz, res, element, sparse=False):
    """-> {"xyz" (n, 3) int64 in vIndex order, "label" (n,) uint32, "size" (c,) uint32, "first" (c,) uint32, "box" (c, 6) uint32}"""
    xyz, _ = _sorted(xyz, None)
    n = len(xyz)
    parent = list(range(n))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    for a, b in (_pairs_sparse if sparse else _pairs_searchsorted)(xyz, res, element).tolist():
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)
    root = np.array([find(v) for v in range(n)], np.int64)
    first = np.flatnonzero(root == np.arange(n))  # the root is the lowest vIndex of its component: ascending = order of first appearance
    label = np.searchsorted(first, root)
    size = np.bincount(label, minlength=len(first))
    box = np.zeros((len(first), 6), np.int64)
    for c in range(len(first)):
        p = xyz[label == c]
        box[c, :3], box[c, 3:] = p.min(0), p.max(0)
    return {"xyz": xyz, "label": label.astype(np.uint32), "size": size.astype(np.uint32), "first": first.astype(np.uint32), "box": box.astype(np.uint32)}


def kept_components(size, min_voxels=1, keep_largest=0):
    """bool per component"""
    size = np.asarray(size, np.int64)
    order = np.lexsort((np.arange(len(size)), -size))  # size descending, then label ascending
    rank = np.empty(len(size), np.int64)
    rank[order] = np.arange(len(size))
    return (size >= min_voxels) & ((rank < keep_largest) if keep_largest else True)


def _split(xyz, attribs, res, element, min_voxels, keep_largest, sparse):
    sx, sa = _sorted(xyz, attribs)
    c = components(sx, res, element, sparse)
    stays = kept_components(c["size"], min_voxels, keep_largest)[c["label"]]
    return sx, sa, stays


def keep(xyz, attribs, res, element, min_voxels=1, keep_largest=0, sparse=False):
    """the surviving (xyz, attribs) in vIndex order, every byte as it was"""
    sx, sa, stays = _split(xyz, attribs, res, element, min_voxels, keep_largest, sparse)
    return sx[stays], sa[stays]


def dropped(xyz, res, element, min_voxels=1, keep_largest=0, sparse=False):
    """the voxels of the components that go, (n, 3) int64: what edit_voxels is given with VOXEL_REMOVE"""
    sx, _, stays = _split(xyz, None, res, element, min_voxels, keep_largest, sparse)
    return sx[~stays]
