"""numpy model of the dilation, erosion, closing and opening of a voxel set (include/mvrt.h, mvrt_svo_dilation_cells / _erosion_voxels / _dilate / _erode / _close /
_open), written from the definitions alone.  No scipy.

Grid [0, R)^3, A the voxel set, element FACES (6 face neighbours) or CUBE (26 neighbours of the 3x3x3 block), N(c) = the neighbours of c inside the grid.
  dilation step  D(A) = A + { c in the grid, not in A, N(c) meets A }; a new cell takes per channel R, G, B of colour and of emission
                 floor( sum over N(c) & A / their number ), both alpha bytes 255; voxels of A keep their 8 bytes
  erosion step   E(A) = { v in A : N(v) lies in A }: outside the grid counts as occupied; the survivors keep their 8 bytes
  k steps        the single step k times, attributes of step i from the set after step i - 1
  closing        k dilation steps, then k erosion steps
  opening        the set of k erosion steps, then k dilation steps, every voxel of it with its ORIGINAL bytes
Everything is listed in ascending Morton code (x = bit 0 of each group), which is the vIndex order of the octree.

The dense form works on boolean grids cropped to the voxels' box grown by `steps` (like fill_expected._box); the sparse form (sparse=True) on Python sets, for a
handful of voxels at gridRes 2^21."""
import numpy as np

from surface_expected import morton

FACES, CUBE = 0, 1
OFFSETS = {
    FACES: [(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)],
    CUBE: [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)],
}
CHANNELS = (0, 1, 2, 4, 5, 6)  # R, G, B of colour and of emission; bytes 3 and 7 are the alphas


def _sorted(xyz, attribs):
    xyz = np.asarray(xyz, np.int64).reshape(-1, 3)
    attribs = np.full((len(xyz), 8), 255, np.uint8) * np.array([1, 1, 1, 1, 0, 0, 0, 1], np.uint8) if attribs is None else np.asarray(attribs, np.uint8).reshape(-1, 8)
    codes = morton(xyz)
    assert len(np.unique(codes)) == len(codes), "the model takes a voxel SET"
    order = np.argsort(codes, kind="stable")
    return xyz[order], attribs[order]


# ---- dense ---------------------------------------------------------------------------------------------------------------------------------------------------
class _Dense:
    def __init__(self, xyz, attribs, res, grow):
        self.res = res
        self.lo = np.maximum(xyz.min(0) - grow, 0)
        self.hi = np.minimum(xyz.max(0) + grow, res - 1)
        shape = tuple(self.hi - self.lo + 1)
        assert max(shape) <= 2048 and np.prod(shape) <= 1 << 24
        self.occ = np.zeros(shape, bool)
        self.attr = np.zeros(shape + (8,), np.uint8)
        p = xyz - self.lo
        self.occ[p[:, 0], p[:, 1], p[:, 2]] = True
        self.attr[p[:, 0], p[:, 1], p[:, 2]] = attribs

    def _shifted(self, padded, d):
        """b[c] = padded[c + d] over the box"""
        sx, sy, sz = self.occ.shape
        return padded[1 + d[0]:1 + d[0] + sx, 1 + d[1]:1 + d[1] + sy, 1 + d[2]:1 + d[2] + sz]

    def new_cells(self, element):
        """-> (new (bool), attr (.., 8) uint8, count) of one dilation step.  A cell outside the box is empty (inside the grid: the box holds the set grown by
        every step to come) or does not exist (outside the grid): either way it adds nothing."""
        occ = np.pad(self.occ, 1)
        val = np.pad(self.attr.astype(np.int64), ((1, 1), (1, 1), (1, 1), (0, 0)))  # (0 where there is no voxel)
        cnt = np.zeros(self.occ.shape, np.int64)
        sums = np.zeros(self.occ.shape + (8,), np.int64)
        for d in OFFSETS[element]:
            cnt += self._shifted(occ, d)
            sums += self._shifted(val, d)
        new = ~self.occ & (cnt > 0)
        attr = np.zeros(self.occ.shape + (8,), np.uint8)
        attr[new] = (sums[new] // cnt[new][:, None]).astype(np.uint8)
        attr[new, 3] = attr[new, 7] = 255
        return new, attr, cnt

    def dilate(self, element):
        new, attr, _ = self.new_cells(element)
        self.occ |= new
        self.attr[new] = attr[new]

    def kept(self, element):
        """the voxels one erosion step keeps.  Outside the grid counts as occupied; outside the box but inside the grid there is no voxel."""
        occ = np.pad(self.occ, 1)
        for axis in range(3):
            s = [slice(None)] * 3
            if self.lo[axis] == 0:
                s[axis] = 0
                occ[tuple(s)] = True
            if self.hi[axis] == self.res - 1:
                s[axis] = -1
                occ[tuple(s)] = True
        keep = self.occ.copy()
        for d in OFFSETS[element]:
            keep &= self._shifted(occ, d)
        return keep

    def erode(self, element):
        keep = self.kept(element)
        self.attr[self.occ & ~keep] = 0
        self.occ = keep

    def listing(self, mask=None):
        q = np.argwhere(self.occ if mask is None else mask)
        order = np.argsort(morton(q + self.lo), kind="stable")
        return q[order]

    def voxels(self):
        q = self.listing()
        return (q + self.lo).astype(np.uint32).reshape(-1, 3), self.attr[q[:, 0], q[:, 1], q[:, 2]].reshape(-1, 8)


# ---- sparse --------------------------------------------------------------------------------------------------------------------------------------------------
class _Sparse:
    def __init__(self, xyz, attribs, res, grow):
        self.res = res
        self.vox = {tuple(int(v) for v in p): np.array(a, np.uint8) for p, a in zip(xyz, attribs)}

    def _neighbours(self, c, element):
        for d in OFFSETS[element]:
            n = (c[0] + d[0], c[1] + d[1], c[2] + d[2])
            if all(0 <= v < self.res for v in n):
                yield n

    def new_cells_dict(self, element):
        cells = {}
        for c in self.vox:
            for n in self._neighbours(c, element):
                if n not in self.vox:
                    cells.setdefault(n, []).append(self.vox[c].astype(np.int64))
        out = {}
        for n, srcs in cells.items():
            a = (np.sum(srcs, axis=0) // len(srcs)).astype(np.uint8)
            a[3] = a[7] = 255
            out[n] = (a, len(srcs))
        return out

    def dilate(self, element):
        for n, (a, _) in self.new_cells_dict(element).items():
            self.vox[n] = a

    def erode(self, element):
        self.vox = {c: a for c, a in self.vox.items() if all(n in self.vox for n in self._neighbours(c, element))}

    def voxels(self):
        if not self.vox:
            return np.zeros((0, 3), np.uint32), np.zeros((0, 8), np.uint8)
        xyz = np.array(list(self.vox), np.int64)
        order = np.argsort(morton(xyz), kind="stable")
        return xyz[order].astype(np.uint32), np.array(list(self.vox.values()), np.uint8)[order]


# ---- the calls -----------------------------------------------------------------------------------------------------------------------------------------------
def dilation_cells(xyz, attribs, res, element, sparse=False):
    """-> {xyz (n, 3) uint32 ascending Morton, attribs (n, 8) uint8, count (n,) uint32}: the cells one dilation step adds"""
    xyz, attribs = _sorted(xyz, attribs)
    if sparse:
        cells = _Sparse(xyz, attribs, res, 1).new_cells_dict(element)
        q = np.array(list(cells), np.int64).reshape(-1, 3)
        order = np.argsort(morton(q), kind="stable")
        at = np.array([v[0] for v in cells.values()], np.uint8).reshape(-1, 8)[order]
        cnt = np.array([v[1] for v in cells.values()], np.uint32)[order]
        return {"xyz": q[order].astype(np.uint32), "attribs": at, "count": cnt}
    g = _Dense(xyz, attribs, res, 1)
    new, attr, cnt = g.new_cells(element)
    q = g.listing(new)
    return {"xyz": (q + g.lo).astype(np.uint32).reshape(-1, 3), "attribs": attr[q[:, 0], q[:, 1], q[:, 2]].reshape(-1, 8),
            "count": cnt[q[:, 0], q[:, 1], q[:, 2]].astype(np.uint32)}


def erosion_voxels(xyz, res, element, sparse=False):
    """-> (n,) uint32: the vIndex (Morton rank), ascending, of the voxels one erosion step removes"""
    xyz, attribs = _sorted(xyz, None)
    after, _ = morph("erode", xyz, attribs, res, element, 1, sparse)
    return np.flatnonzero(~np.isin(morton(xyz), morton(after))).astype(np.uint32)


def morph(op, xyz, attribs, res, element, steps, sparse=False):
    """op in dilate / erode / close / open -> (xyz (n, 3) uint32 ascending Morton, attribs (n, 8) uint8).  An erosion may leave nothing: the calls refuse that,
    the model returns the empty set."""
    xyz, attribs = _sorted(xyz, attribs)
    g = (_Sparse if sparse else _Dense)(xyz, attribs, res, steps)
    for half in {"dilate": "d", "erode": "e", "close": "de", "open": "ed"}[op]:
        for _ in range(steps):
            g.dilate(element) if half == "d" else g.erode(element)
    out, at = g.voxels()
    if op == "open" and len(out):  # a pure removal: the original bytes
        index = {int(c): i for i, c in enumerate(morton(xyz))}
        at = attribs[[index[int(c)] for c in morton(out)]]
    return out, at
