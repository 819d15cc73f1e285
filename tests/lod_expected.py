"""What the cone-limited walk of include/mvrt/device.hpp (mvrt::DeviceOctree::walk<false, true>, intersectCone) must give, for tests/test_cone_walk_cpu.py (the
header built for the host, tests/cpp/cone_walk_host.cpp) and tests/test_gpu_cone.py (mvrt_trace_batch_cone, tests/hip/cone_probe.hip, mvrt_render_primary_lod).

The model is a scalar np.float32 port of the walk, one operation per rounding, on a POINTER-FREE octree: per level the set of occupied Morton prefixes
(code >> 3 * (levels - level)).  No node array, no DAG, no flavour: a child exists when its prefix is in the next level's set.  With the cone off it must equal
the oracle's Scene.trace in t, nMajor and descents on every ray it is used on (validate); only then is its cone rule believed:

    on the FIRST visit of an inner node at level in [1, levels - 1], entered at S = max3(tx0, ty0, tz0): f = coneA + coneB * S (two roundings); the node is
    terminal iff 0 < S and dps * 2^levels * 2^-level <= f, and reports t = S, nMajor by the voxel's rule, level, cellCode = its prefix.

Everything is computed once per scene and frozen."""
import os
import struct

import numpy as np

import coarsen_expected as CE
import surface_expected as S
from common import bunny_tris

f32 = np.float32
MAXF = f32(3.402823466e38)
ZERO, HALF, ONE = f32(0), f32(0.5), f32(1)
N_RAYS = 4096
# coneA and coneB of the rays cycle over the 36 pairs of these (2^-9 is pixel-like: one pixel of a 512-pixel image at unit distance) and the fixed depths (cones)
CONE_VALUES = (f32(0), f32(2.0 ** -9), f32(2.0 ** -5), f32(np.inf), f32(-1), f32(np.nan))
OUTPUTS = ("t", "nMajor", "level", "cellCode", "descents")
TYPES = (np.float32, np.int32, np.uint32, np.uint64, np.uint32)
MAGIC = 0x454E4F43


def smax(x, y):  # the header's ternaries, argument order included
    return y if x < y else x


def smin(x, y):
    return y if y < x else x


def sabs(x):
    return x if x >= ZERO else -x


def max3(a, b, c):
    return smax(smax(a, b), c)


def min3(a, b, c):
    return smin(smin(a, b), c)


class Prefixes:
    """the pointer-free octree of a voxel set: occ[level] = the occupied prefixes of that level, level in [1, levels]"""

    def __init__(self, codes, levels, lower, upper, dps):
        codes = np.asarray(codes, np.uint64)
        self.levels = int(levels)
        self.occ = [None] + [set((codes >> np.uint64(3 * (self.levels - l))).tolist()) for l in range(1, self.levels + 1)]
        self.lower = [f32(v) for v in lower]
        self.upper = [f32(v) for v in upper]
        root_edge = f32(dps) * f32(2.0 ** self.levels)
        self.size = [root_edge * f32(2.0 ** -l) for l in range(self.levels + 1)]
        self.scale = [f32(2.0 ** -l) for l in range(self.levels + 1)]


def walk(tree, ro, rd, cone_a, cone_b, cone=True):
    """one ray -> (t, nMajor, level, cellCode, descents); ro, rd: three np.float32 each"""
    lo, hi, levels, occ = tree.lower, tree.upper, tree.levels, tree.occ
    o = [ro[0], ro[1], ro[2]]
    inv = [ONE / rd[0], ONE / rd[1], ONE / rd[2]]
    vmask = 0
    for k in range(3):
        if inv[k] < ZERO:
            vmask |= 1 << k
            inv[k] = -inv[k]
            o[k] = lo[k] + hi[k] - o[k]
    for k in range(3):
        inv[k] = smin(inv[k], MAXF / smax(smax(sabs(lo[k] - o[k]), sabs(hi[k] - o[k])), ONE))
    t0 = [(lo[k] - o[k]) * inv[k] for k in range(3)]
    t1 = [(hi[k] - o[k]) * inv[k] for k in range(3)]
    if min3(*t1) < max3(*t0):
        return MAXF, -1, 0, 0, 0
    dtx, dty, dtz = t1[0] - t0[0], t1[1] - t0[1], t1[2] - t0[2]
    tx1, ty1, tz1 = t1
    level, child_mask, descents, path = 0, 8, 0, 0
    pending = {}  # level -> (path, tx1, ty1, tz1, the candidate it resumes with)
    while True:
        scale = tree.scale[level]
        tx0 = tx1 - dtx * scale
        ty0 = ty1 - dty * scale
        tz0 = tz1 - dtz * scale
        s = max3(tx0, ty0, tz0)
        pop = False
        if level == levels:  # a voxel
            if ZERO < s:
                return s, (1 if s == tx0 else (2 if s == ty0 else 0)), level, path, descents
            pop = True
        else:
            if cone and (child_mask & 8) and 1 <= level < levels:
                f = cone_a + cone_b * s
                if ZERO < s and tree.size[level] <= f:
                    return s, (1 if s == tx0 else (2 if s == ty0 else 0)), level, path, descents
            txm = HALF * (tx0 + tx1)
            tym = HALF * (ty0 + ty1)
            tzm = HALF * (tz0 + tz1)
            if child_mask & 8:
                child_mask = (1 if txm < s else 0) | (2 if tym < s else 0) | (4 if tzm < s else 0)
            x1 = tx1 if child_mask & 1 else txm
            y1 = ty1 if child_mask & 2 else tym
            z1 = tz1 if child_mask & 4 else tzm
            u = min3(x1, y1, z1)
            mv = 1 if u == x1 else (2 if u == y1 else 4)
            has_next = (child_mask & mv) == 0
            child = child_mask ^ vmask
            nxt = child_mask | mv
            if ((path << 3) | child) in occ[level + 1] and not (u < ZERO):
                if has_next:
                    pending[level] = (path, tx1, ty1, tz1, nxt)
                descents += 1
                path = (path << 3) | child
                tx1, ty1, tz1 = x1, y1, z1
                level += 1
                child_mask = 8
            elif has_next:
                child_mask = nxt
            else:
                pop = True
        if pop:
            if not pending:
                return MAXF, -1, 0, 0, descents
            level = max(pending)
            path, tx1, ty1, tz1, child_mask = pending.pop(level)


def trace(tree, ro, rd, cone_a=None, cone_b=None):
    """every ray of (n, 3) float32 arrays -> the OUTPUTS as arrays; cone_a None = the cone off"""
    ro, rd = np.ascontiguousarray(ro, f32).reshape(-1, 3), np.ascontiguousarray(rd, f32).reshape(-1, 3)
    n = len(ro)
    cone = cone_a is not None
    a = np.broadcast_to(np.asarray(cone_a if cone else 0, f32), (n,))
    b = np.broadcast_to(np.asarray(cone_b if cone else 0, f32), (n,))
    out = {k: np.zeros(n, d) for k, d in zip(OUTPUTS, TYPES)}
    with np.errstate(all="ignore"):
        for i in range(n):
            r = walk(tree, ro[i], rd[i], a[i], b[i], cone)
            for k, v in zip(OUTPUTS, r):
                out[k][i] = v
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def cones(n, dps, levels):
    """(coneA, coneB) of n rays: the 36 pairs of CONE_VALUES in turn, then the fixed-depth setting (dps * 2^(levels - D), 0) of every D in [1, levels - 1]"""
    v = np.array(CONE_VALUES, f32)
    pairs = [(v[i // 6], v[i % 6]) for i in range(36)] + [(f32(dps) * f32(2.0 ** (levels - D)), f32(0)) for D in range(1, levels)]
    pairs = np.array(pairs, f32)[np.arange(n) % len(pairs)]
    return pairs[:, 0].copy(), pairs[:, 1].copy()


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------------------------
def position_attribs(xyz, res):
    """a colour and an emission that differ from voxel to voxel: means that forget a voxel, or take one twice, differ"""
    xyz = np.asarray(xyz, np.int64).reshape(-1, 3)
    a = np.zeros((len(xyz), 8), np.uint8)
    a[:, 0] = (xyz[:, 0] * 255) // max(res - 1, 1)
    a[:, 1] = (xyz[:, 1] * 255) // max(res - 1, 1)
    a[:, 2] = (xyz[:, 2] * 255) // max(res - 1, 1)
    a[:, 3] = 255
    a[:, 4] = (xyz[:, 0] * 7 + xyz[:, 1] * 13 + xyz[:, 2] * 29) % 256
    a[:, 5] = (xyz[:, 0] * 31 + xyz[:, 2] * 3) % 256
    a[:, 6] = (xyz[:, 1] * 17) % 256
    a[:, 7] = 255
    return a


HAND_MADE = {
    # name: (gridRes, the voxels).  corner: one voxel in the far corner, alone in every coarse cell.  between: two voxels of one 4^3 cell on a diagonal, a ray can
    # pass between them: the cone hits the cell, the unlimited ray misses.  twins: two 2^3 blocks of equal shape -- one DAG node for both -- in different colours
    "corner": (8, [(7, 7, 7)]),
    "between": (8, [(0, 0, 0), (3, 3, 0), (3, 0, 3), (0, 3, 3)]),
    "twins": (8, [(x, y, z) for x in range(2) for y in range(2) for z in range(2) if (x + y + z) % 2 == 0] +
              [(4 + x, 4 + y, 6 + z) for x in range(2) for y in range(2) for z in range(2) if (x + y + z) % 2 == 0]),
}
HAND_ORIGIN, HAND_DPS = np.array([-0.25, 0.5, 1.0], f32), f32(2.0 ** -4)
DEEP = "deep16"
SCENES = ("bunny2", "bunny4", "bunny8", "bunny32", "bunny64", "corner", "between", "twins")


class LodScene:
    """one voxel set with everything the tests compare against: the oracle's Scene (sc, embedded or plain), the sorted codes with their coordinates and attributes,
    the pointer-free octree, the rays with their cones, the model's answers with the cone off and on, and the pyramid"""

    def __init__(self, O, name, embedded=True, n_rays=N_RAYS):
        self.name, self.embedded = name, embedded
        if name.startswith("bunny"):
            res = int(name[5:])
            sc = O.build_scene_from_triangles(bunny_tris(), res, embed=embedded)
            codes = np.asarray(sc.morton, np.uint64)
            xyz = S.decode(codes)
            attribs = position_attribs(xyz, res)
            sc = O.Scene(sc.nodes, attribs, sc.origin, sc.dps, res, 1, embedded=embedded)
        elif name == DEEP:  # the 16-level scene of tests/lane_walk_expected.py, with its own aimed rays
            import lane_walk_expected as E
            import reference_pins as R
            rs = R.ray_scene(O, name)
            sc = E.oracle_scene(O, name, embedded)
            res, codes, attribs = sc.grid_res, np.asarray(rs.morton, np.uint64), sc.attrs
            xyz = S.decode(codes)
            parts = [rs.deep.short_rays(n_rays // 2, 31)[:2], rs.deep.long_rays(n_rays // 4, 32), rs.deep.tie_rays(n_rays - n_rays // 2 - n_rays // 4, 33)]
            deep_rays = tuple(np.concatenate([p[k] for p in parts]).astype(f32) for k in (0, 1))
        else:
            res, vox = HAND_MADE[name]
            xyz = np.asarray(vox, np.int64)
            codes = S.morton(xyz)
            order = np.argsort(codes)
            codes, xyz = codes[order], xyz[order]
            attribs = position_attribs(xyz, res)
            if name == "twins":
                attribs[:4, :3], attribs[4:, :3] = (200, 40, 10), (10, 60, 220)
            sc = O.Scene(O.build_octree(codes, res, embed=embedded), attribs, HAND_ORIGIN, HAND_DPS, res, 1, embedded=embedded)
        self.sc, self.res, self.levels = sc, res, int(np.log2(res))
        self.codes, self.xyz, self.attribs = np.asarray(codes, np.uint64), np.asarray(xyz, np.uint32).reshape(-1, 3), attribs
        self.lower, self.upper = sc.bounds()
        self.tree = Prefixes(self.codes, self.levels, self.lower, self.upper, sc.dps)
        self.ro, self.rd = deep_rays if name == DEEP else rays(self, n_rays, seed=len(name) * 131 + res)
        self.outside = np.arange(len(self.ro)) < (0 if name == DEEP else len(self.ro) // 2)
        self.cone_a, self.cone_b = cones(len(self.ro), sc.dps, self.levels)
        self.oracle = sc.trace(self.ro, self.rd, None, threads=8, want_descents=True)
        self.off = trace(self.tree, self.ro, self.rd)
        self.on = trace(self.tree, self.ro, self.rd, self.cone_a, self.cone_b)
        for a in (self.codes, self.xyz, self.attribs, self.ro, self.rd, self.outside, self.cone_a, self.cone_b, *self.off.values(), *self.on.values()):
            a.setflags(write=False)

    def validate(self):
        """the model with the cone off IS the oracle: t, nMajor and descents of every ray, bit for bit; a voxel hit names the voxel the oracle's vIndex names"""
        for k in ("t", "nMajor", "descents"):
            same = bits(self.off[k]) == bits(self.oracle[k])
            assert same.all(), "%s: the model's %s differs from the oracle on %d of %d rays, first at %d" % (self.name, k, (~same).sum(), same.size, np.argmax(~same))
        hit = self.off["t"] != MAXF
        assert (self.off["level"][hit] == self.levels).all() and (self.off["level"][~hit] == 0).all()
        assert np.array_equal(self.codes[self.oracle["vIndex"][hit]], self.off["cellCode"][hit])
        return int(hit.sum())

    def level(self, L):
        """level L of the pyramid: {code, attribs, count} from the numpy model of the coarsening"""
        c = CE.coarse(self.xyz, self.attribs, self.levels - L)
        return {"code": S.morton(c["xyz"].astype(np.int64)), "attribs": c["attribs"], "count": c["count"]}

    def attrib_of(self, out):
        """(index, attribs) the pyramid holds for the hits of `out`: the rank of the cell in its level and its mean attribute, a voxel's own at the last level;
        zeros on a miss"""
        n = len(out["t"])
        index, attribs = np.zeros(n, np.uint32), np.zeros((n, 8), np.uint8)
        for L in range(1, self.levels + 1):
            sel = np.flatnonzero(out["level"] == L)
            lv = {"code": self.codes, "attribs": self.attribs} if L == self.levels else self.level(L)
            pos = np.searchsorted(lv["code"], out["cellCode"][sel])
            assert np.array_equal(lv["code"][pos], out["cellCode"][sel])
            index[sel], attribs[sel] = pos, lv["attribs"][pos]
        return index, attribs

    def coarse_scene(self, O, D):
        """the oracle's Scene of the octree coarsened to D levels: the unique codes >> 3 (levels - D) at gridRes >> (levels - D), same origin, dps * 2^(levels - D)"""
        k = self.levels - D
        cells = np.unique(self.codes >> np.uint64(3 * k))
        sc = O.Scene(O.build_octree(cells, self.res >> k, embed=True), np.zeros((len(cells), 8), np.uint8), self.sc.origin, f32(self.sc.dps) * f32(2.0 ** k), self.res >> k)
        lo, hi = sc.bounds()
        assert np.array_equal(lo, self.lower) and np.array_equal(hi, self.upper)
        return sc, cells


def rays(sc, n, seed):
    """n rays, the first half from outside the root box by at least a quarter extent (aimed at voxels and at random points of the box, a fifth of them with one or two
    zero direction components), the second half from inside the grid: a half of those from inside a voxel"""
    rng = np.random.default_rng(seed)
    lo, ext = sc.lower.astype(np.float64), float(f32(sc.sc.dps) * f32(sc.res))
    dps = float(sc.sc.dps)
    centre = lo + 0.5 * ext
    h = n // 2

    def targets(m):
        vox = lo + (sc.xyz[rng.integers(0, len(sc.xyz), m)] + rng.random((m, 3))) * dps
        anywhere = lo + rng.random((m, 3)) * ext
        return np.where(rng.random((m, 1)) < 0.7, vox, anywhere)

    tgt = targets(h)
    ro = centre + (rng.random((h, 3)) - 0.5) * 3.0 * ext
    axis, sign = rng.integers(0, 3, h), rng.choice([-1.0, 1.0], h)
    ro[np.arange(h), axis] = centre[axis] + sign * (0.75 + 0.75 * rng.random(h)) * ext  # outside by a quarter extent at least
    z = h // 5
    free = [(axis[i],) if i % 2 else (axis[i], (axis[i] + 1) % 3) for i in range(z)]  # the components that stay: one or two
    for i in range(z):  # zero components: the origin moves onto the target along the others
        for k in range(3):
            if k not in free[i]:
                ro[i, k] = tgt[i, k]
    outside = (ro.astype(f32), (tgt - ro).astype(f32))
    for i in range(z):
        for k in range(3):
            if k not in free[i]:
                outside[1][i, k] = 0.0
    m = n - h
    inside = lo + rng.random((m, 3)) * ext
    v = m // 2
    inside[:v] = lo + (sc.xyz[rng.integers(0, len(sc.xyz), v)] + 0.25 + 0.5 * rng.random((v, 3))) * dps  # inside a voxel
    d = rng.standard_normal((m, 3))
    d[::7, 0] = 0.0
    d[3::11, 1] = 0.0
    d[5::13, 2] = 0.0
    ro = np.concatenate([outside[0], inside.astype(f32)])
    rd = np.concatenate([outside[1], d.astype(f32)])
    big = np.abs(ro[:h] - centre.astype(f32)).max(1)
    assert (big >= f32(0.74 * ext)).all()
    return ro, rd


_scenes = {}


def scene(O, name, embedded=True):
    if (name, embedded) not in _scenes:
        _scenes[(name, embedded)] = LodScene(O, name, embedded)
    return _scenes[(name, embedded)]


# ---- the input and output files of tests/cpp/cone_walk_host.cpp -----------------------------------------------------------------------------------------
def write_input(path, view_bytes, lines, masks, psum_cold, stack_mode, ro, rd, cone_a, cone_b):
    """view_bytes: the 128 bytes of an mvrt_device_octree (its pointers are set by the program); plain flavour: masks and psum_cold, else None"""
    with open(path, "wb") as f:
        f.write(struct.pack("<4I2Q", MAGIC, stack_mode, 0, 0, len(lines), len(ro)))
        f.write(view_bytes)
        f.write(lines.tobytes())
        if masks is not None:
            f.write(masks.tobytes())
            f.write(psum_cold.tobytes())
        for a in (ro, rd, cone_a, cone_b):
            f.write(np.ascontiguousarray(a, f32).tobytes())
    return len(ro)


def read_output(path, n):
    """-> (intersectConeEx, intersectCone): the OUTPUTS of the first, the first four of the second"""
    raw = np.fromfile(path, np.uint8)
    assert len(raw) == n * (24 + 20), (len(raw), n)
    out, p = [], 0
    for keys in (OUTPUTS, OUTPUTS[:4]):
        d = {}
        for k in keys:
            ty = np.dtype(TYPES[OUTPUTS.index(k)])
            d[k] = raw[p:p + n * ty.itemsize].view(ty)
            p += n * ty.itemsize
        out.append(d)
    return out


CONE_WALK_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "cone_walk_host.cpp")
