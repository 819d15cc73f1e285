"""Seeded voxel sets and ray sets for octrees of 14 to 21 levels (tests/test_deep_octree_cpu.py, tests/test_gpu_deep_octree.py).

Random voxels in a 2^21 grid are almost never hit by random rays, so a deep scene is a few dense clusters (a solid 16^3 block on the
grid's lowest corner, a one-voxel-thick 64 x 64 plate on its highest corner, a hollow sphere shell of radius 20 in the middle and a
second solid block) plus a few thousand isolated voxels (single-child chains from near the root down to the last level).  The ray sets
aim at them.  The grid is the unit cube: origin 0 and dps = 2^-L are exact in float32.  (Not a wider one: where the grid is wider than
max(|lower - ro|, |upper - ro|, 1), the reference's clamp of 1 / 0 (voxCommon.hpp:265-269) lets the root's t range of a zero direction
component overflow to inf, and an axis-parallel ray no longer follows its own coordinate on that axis: DESIGN.md 3, "Precision at depth".)"""
import numpy as np

f32 = np.float32
DEPTHS = (14, 15, 16, 17, 20, 21)
ORIGIN = np.array([0.0, 0.0, 0.0], np.float32)
N_ISOLATED = 3000
KIND_AXIS, KIND_TILTED, KIND_GENERAL = 0, 1, 2


def part1by2(v):
    """the 21 low bits of v spread to every third bit (numpy, independent of the oracle's encoder)"""
    v = np.asarray(v, np.uint64) & np.uint64(0x1FFFFF)
    for shift, mask in ((32, 0x1F00000000FFFF), (16, 0x1F0000FF0000FF), (8, 0x100F00F00F00F00F), (4, 0x10C30C30C30C30C3), (2, 0x1249249249249249)):
        v = (v | (v << np.uint64(shift))) & np.uint64(mask)
    return v


def morton(xyz):
    """(n, 3) integer coordinates -> Morton codes (x = bit 0)"""
    xyz = np.asarray(xyz).reshape(-1, 3)
    return part1by2(xyz[:, 0]) | (part1by2(xyz[:, 1]) << np.uint64(1)) | (part1by2(xyz[:, 2]) << np.uint64(2))


def decode(m):
    """Morton codes -> (n, 3) uint32"""
    m = np.asarray(m, np.uint64)
    out = np.zeros((len(m), 3), np.uint32)
    for axis in range(3):
        v = np.zeros(len(m), np.uint64)
        for b in range(21):
            v |= ((m >> np.uint64(3 * b + axis)) & np.uint64(1)) << np.uint64(b)
        out[:, axis] = v.astype(np.uint32)
    return out


def dps_of(levels):
    return f32(1.0 / (1 << levels))


def _shell(centre, r):
    k = np.arange(-r - 1, r + 2)
    g = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3)
    d = np.sqrt(((g + 0.5) ** 2).sum(1))
    return g[(d >= r - 0.5) & (d < r + 0.5)] + centre


def clusters(levels):
    """the dense clusters of a scene of `levels` levels: {name: (n, 3) int64}"""
    res = 1 << levels
    k16 = np.arange(16)
    block = np.stack(np.meshgrid(k16, k16, k16, indexing="ij"), -1).reshape(-1, 3)
    k64 = np.arange(res - 64, res)
    plate = np.stack(np.meshgrid(k64, k64, [res - 1], indexing="ij"), -1).reshape(-1, 3)
    centre = np.array([int(res * 0.375) + 5, int(res * 0.625) - 3, int(res * 0.53)], np.int64)
    shell = _shell(centre, 20)
    block2 = block + np.array([int(res * 0.6), int(res * 0.3) + 7, int(res * 0.45) - 2])
    return {"block": block.astype(np.int64), "plate": plate.astype(np.int64), "shell": shell.astype(np.int64), "block2": block2.astype(np.int64)}


class DeepScene:
    """xyz (n, 3) uint32 with duplicates and random order, attrs (n, 8) uint8; sorted unique codes `morton` for the lookups"""

    def __init__(self, levels, seed=None):
        self.levels = levels
        self.res = 1 << levels
        self.origin = ORIGIN.copy()
        self.dps = dps_of(levels)
        rng = np.random.default_rng(1000 + levels if seed is None else seed)
        self.clusters = clusters(levels)
        iso = rng.integers(0, self.res, size=(N_ISOLATED, 3))
        pts = np.concatenate(list(self.clusters.values()) + [iso])
        pts = np.concatenate([pts, pts[rng.integers(0, len(pts), 500)]])  # duplicates merge
        pts = pts[rng.permutation(len(pts))]
        self.xyz = pts.astype(np.uint32)
        attrs = rng.integers(0, 256, size=(len(pts), 8), dtype=np.uint8)
        attrs[rng.random(len(pts)) >= 0.15, 4:7] = 0  # emission on a minority
        self.attrs = attrs
        self.morton = np.unique(morton(self.xyz))

    def occupied(self, cells):
        """(n, 3) int64 cells -> bool: the cell holds a voxel (cells outside the grid never do)"""
        cells = np.asarray(cells, np.int64).reshape(-1, 3)
        inside = ((cells >= 0) & (cells < self.res)).all(1)
        code = morton(np.where(inside[:, None], cells, 0))
        i = np.minimum(np.searchsorted(self.morton, code), len(self.morton) - 1)
        return inside & (self.morton[i] == code)

    def to_world(self, p):
        """voxel units (float64) -> world float32"""
        return (self.origin.astype(np.float64) + np.asarray(p, np.float64) * float(self.dps)).astype(np.float32)

    def to_voxel(self, p):
        """world float32 -> voxel units float64 (exact: dps is a power of two)"""
        return (np.asarray(p, np.float32).astype(np.float64) - self.origin.astype(np.float64)) / float(self.dps)

    # ---- rays ----------------------------------------------------------------------------------------------------------------------------
    def short_rays(self, n, seed):
        """rays from an empty cell 1-8 voxels in front of a face of a target voxel whose neighbour across that face is empty.  Returns
        ro, rd (float32 world), kind (KIND_AXIS: along the face normal, KIND_TILTED: normal + 1e-3 noise, KIND_GENERAL: to a random point of
        the target or of the voxel next to it), target (n, 3) int64"""
        rng = np.random.default_rng(seed)
        vox = decode(self.morton).astype(np.int64)
        m = 4 * n
        tgt = vox[rng.integers(0, len(vox), m)]
        axis = rng.integers(0, 3, m)
        sign = np.where(rng.random(m) < 0.5, -1, 1)
        e = np.zeros((m, 3), np.int64)
        e[np.arange(m), axis] = sign
        ok = ~self.occupied(tgt + e)
        dist = 1.0 + 7.0 * rng.random(m)
        p = tgt + 0.1 + 0.8 * rng.random((m, 3))
        face = tgt[np.arange(m), axis] + (sign > 0)
        p[np.arange(m), axis] = face + sign * dist
        ro = self.to_world(p)
        ok &= ~self.occupied(np.floor(self.to_voxel(ro)).astype(np.int64))
        ok &= ((p >= 0) & (p < self.res)).all(1)
        idx = np.flatnonzero(ok)[:n]
        ro, tgt, axis, sign = ro[idx], tgt[idx], axis[idx], sign[idx]
        k = len(idx)
        kind = np.arange(k) % 3
        rd = np.zeros((k, 3), np.float64)
        rd[np.arange(k), axis] = -sign
        tilt = kind == KIND_TILTED
        rd[tilt] += 1e-3 * rng.normal(size=(tilt.sum(), 3))
        gen = kind == KIND_GENERAL
        aim = tgt[gen] + rng.random((gen.sum(), 3))
        aim[::4] += rng.integers(-1, 2, size=aim[::4].shape)  # a quarter aim next to the target: near misses and other voxels
        rd[gen] = aim - self.to_voxel(ro[gen])
        rd /= np.linalg.norm(rd, axis=1, keepdims=True)
        return ro, rd.astype(np.float32), kind, tgt

    def long_rays(self, n, seed):
        """camera-like rays from outside the grid onto random points of the clusters' voxels"""
        rng = np.random.default_rng(seed)
        pts = np.concatenate(list(self.clusters.values()))
        tgt = pts[rng.integers(0, len(pts), n)] + rng.random((n, 3))
        u = rng.normal(size=(n, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        tw = self.to_world(tgt).astype(np.float64)
        ro = (tw + 1.8 * u).astype(np.float32)
        rd = (tw - ro).astype(np.float32)
        k = n // 10
        rd[:k, 0] = 0.0
        rd[k:2 * k, 1] = 0.0
        rd[2 * k:3 * k, 2] = 0.0
        return ro, rd

    def tie_rays(self, n, seed):
        """like tests/rays.py's tie_rays at the deep levels: diagonals through lattice points (cell corners of the last 6 levels)
        next to the clusters from dyadic distances outside the grid, and from ON those lattice points"""
        rng = np.random.default_rng(seed)
        pts = np.concatenate(list(self.clusters.values()))
        dirs = np.array([(1, 1, 1), (1, 1, -1), (1, -1, 1), (-1, 1, 1), (1, 1, 0.5), (1, 0.5, 1), (0.5, 1, 1), (1, 0.5, 0.25), (2, 1, 1), (1, 2, -1),
                         (-1, -1, -1), (1, -1, -0.5)], np.float32)
        cell = (1 << rng.integers(0, 6, n)).astype(np.int64)
        p = (pts[rng.integers(0, len(pts), n)] + rng.integers(0, 2, (n, 3))) // cell[:, None] * cell[:, None]
        pw = self.to_world(p)
        d = dirs[np.arange(n) % len(dirs)]
        s = (2.0 ** rng.integers(0, 3, n)).astype(np.float32)
        ro = (pw - d * s[:, None]).astype(np.float32)
        on = np.arange(n) % 3 == 0
        ro[on] = pw[on]
        rd = np.where((np.arange(n) % 3 == 1)[:, None], d * f32(0.5), d).astype(np.float32)
        return ro, rd

    def camera(self, target="shell", distance=300.0, res_w=128, res_h=96):
        """a pinhole camera inside the grid `distance` voxels from a cluster's centre, looking at it (CameraPinhole: o, front, up, right,
        tanHthetaY, lensR, focus)"""
        c = self.clusters[target].mean(0) + 0.5
        eye = c + np.array([0.6, 0.35, 0.72]) * distance / np.linalg.norm([0.6, 0.35, 0.72])
        o = self.to_world(eye)
        front = (self.to_world(c).astype(np.float64) - o.astype(np.float64))
        front = (front / np.linalg.norm(front)).astype(np.float32)
        right = np.array([-front[2], 0.0, front[0]], np.float32)
        right = (right / np.float32(np.linalg.norm(right))).astype(np.float32)
        up = np.cross(right, front).astype(np.float32)
        cam = np.zeros(15, np.float32)
        cam[0:3], cam[3:6], cam[6:9], cam[9:12] = o, front, up, right
        cam[12], cam[13], cam[14] = f32(np.tan(np.radians(10.0))), 0.0, 1.0
        return cam


_cache = {}


def scene(levels):
    if levels not in _cache:
        _cache[levels] = DeepScene(levels)
    return _cache[levels]


def oracle_scene(O, s, flags=0):
    """O.merge_voxels -> O.build_octree -> O.Scene for a DeepScene; flags as mvrt's: 1 = no DAG, 2 = masks not embedded"""
    m, a, he = O.merge_voxels(O.morton_encode_batch(s.xyz), s.attrs)
    embed = not (flags & 2)
    nodes = O.build_octree(m, s.res, dag=not (flags & 1), embed=embed)
    sc = O.Scene(nodes, a, s.origin, s.dps, s.res, he, embedded=embed)
    sc.morton = m
    return sc
