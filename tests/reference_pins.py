"""Inputs, fixtures and the comparison rule of the pins against the COMPILED reference (oracle/_ref/libmvrt_ref_walk.so, built by `make -C oracle ref`
from voxCommon.hpp, voxelization.hpp, morton.hpp and IntersectorOctree.hpp as they lie): tests/test_reference_pins_cpu.py (oracle == reference) and
tests/test_gpu_reference_pins.py (kernels == reference).

Where oracle/_ref is absent, the reference's answers are still known: a SHA-256 of each answer is stored in tests/golden/reference_pin_digests.json
(tools/make_reference_pin_digests.py, run where the reference builds), and the side under test must reproduce it -- the way the morton / Murmur pins keep
their stored vectors.  Every comparison is exact: integers as they are, floats by their bits."""
import hashlib
import json
import os

import numpy as np

import deep_scenes as D
from common import GOLDEN, bunny_tris

f32 = np.float32
MAXF = f32(3.402823466e38)
DIGESTS = os.path.join(GOLDEN, "reference_pin_digests.json")
REFERENCE_TREE = os.environ.get("MVRT_REFERENCE", "/root/reference")


# ---- the compiled reference, or its stored answers ---------------------------------------------------------------------------------------------
def load_walk(O, tree_decides):
    """The RefWalk of oracle/_ref, or None.  tree_decides: where the reference tree is present, a missing library is a failure (CPU tests); GPU
    tests never look at the tree, for them a half-built oracle/_ref is the failure."""
    ref = O.load_ref()
    if tree_decides and os.path.isdir(REFERENCE_TREE):
        assert ref is not None and ref.walk is not None, "the reference tree is present but oracle/_ref is not built: run __graft_entry__.build() (make -C oracle ref)"
    if ref is None:
        return None
    assert ref.walk is not None, "oracle/_ref holds libmvrt_ref.so but not libmvrt_ref_walk.so: rebuild it (make -C oracle ref)"
    return ref.walk


def bits(a):
    """an array as the integers of its bytes: floats compare bit for bit, NaN payloads and the sign of zero included"""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(("%s%s;" % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


_stored = None
_record = None  # tools/make_reference_pin_digests.py sets a dict: check() then stores the reference's digests instead of asserting them


def stored():
    global _stored
    if _stored is None:
        with open(DIGESTS) as f:
            _stored = json.load(f)
    return _stored


def check(key, got, walk, reference):
    """got: the arrays of the side under test.  reference(walk) -> the same arrays from the compiled reference.  With the library: every array equal
    bit for bit, and the reference's digest is the stored one (the fixture is current).  Without: the digest of `got` is the stored one."""
    if walk is None:
        assert digest(got) == stored()[key], key + ": differs from the compiled reference's stored answer"
        return
    want = reference(walk)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (key, k, g.dtype, w.dtype, g.shape, w.shape)
        same = bits(g) == bits(w)
        assert same.all(), "%s: array %d differs from the compiled reference at %d of %d entries, first at %s" % (key, k, (~same).sum(), same.size,
                                                                                                                  np.argwhere(~same)[0])
    if _record is not None:
        _record[key] = digest(want)
        return
    assert digest(want) == stored().get(key), key + ": tests/golden/reference_pin_digests.json is stale (tools/make_reference_pin_digests.py)"


def node_fields(nodes, psum=True):
    return [nodes["mask"], nodes["children"]] + ([nodes["psum"]] if psum else [])


# ---- adversarial triangles -----------------------------------------------------------------------------------------------------------------------
CLASSES = ("lattice", "in_plane", "two_equal", "sliver", "clipped", "generic", "sub_voxel")
EXTENT = 8.0  # the grid of the triangle classes: origin 0, dps = EXTENT / res (0.25 at 32^3, 2 at 4^3, 2^-8 at 2048^3: lattice points are exact)


def class_grid(res):
    return np.zeros(3, f32), f32(EXTENT / res)


def triangle_classes(res, n=300, seed=0, span=None, origin=None, dps=None):
    """{class: (n, 9) float32}: n triangles per class in a res^3 grid, each within `span` voxels (default min(res, 24): a 2048^3 grid gets small
    triangles anywhere, far corner included, not 300 walls of millions of voxels).  Coordinates are made in voxel units and scaled by a power-of-two
    dps, so integer coordinates ARE lattice points of the grid in float32.
      lattice    every vertex on a lattice point
      in_plane   axis-aligned: the triangle lies in a lattice plane (a third of them with lattice vertices as well)
      two_equal  two vertices equal (zero normal: kx, ky are NaN)
      sliver     the third vertex (nearly, a quarter: exactly) on the line through the other two
      clipped    partly or wholly outside the grid
      generic    anything
      sub_voxel  smaller than a voxel"""
    o, d = class_grid(res)
    origin = o if origin is None else np.asarray(origin, f32)
    dps = d if dps is None else f32(dps)
    rng = np.random.default_rng(1000 * seed + res)
    span = min(res, 24) if span is None else span

    def base():
        return rng.integers(0, res - span + 1, (n, 1, 3)).astype(np.float64)

    def generic():
        return base() + rng.random((n, 3, 3)) * span

    out = {"lattice": base() + rng.integers(0, span + 1, (n, 3, 3))}
    t = generic()
    t[::3] = np.round(t[::3])
    axis = rng.integers(0, 3, n)
    t[np.arange(n), :, axis] = np.round(t[np.arange(n), 0, axis])[:, None]
    out["in_plane"] = t
    t = generic()
    w = np.arange(n) % 3
    t[np.arange(n), (w + 1) % 3] = t[np.arange(n), w]
    out["two_equal"] = t
    t = generic()
    u = rng.random((n, 1)) * 1.2 - 0.1
    t[:, 2] = t[:, 0] + (t[:, 1] - t[:, 0]) * u + rng.normal(size=(n, 3)) * 1e-4 * (np.arange(n) % 4 != 0)[:, None]
    out["sliver"] = t
    out["clipped"] = rng.integers(-span, res, (n, 1, 3)) + rng.random((n, 3, 3)) * span * 1.5
    out["generic"] = generic()
    out["sub_voxel"] = rng.random((n, 1, 3)) * res + (rng.random((n, 3, 3)) - 0.5) * 0.6
    return {k: (origin.astype(np.float64) + v * float(dps)).astype(f32).reshape(n, 9) for k, v in out.items()}


def one_generic_triangle(res, origin=None, dps=None):
    """a fixed ordinary triangle across the middle of the grid: a mesh of a degenerate class plus this one still touches voxels"""
    o, d = class_grid(res)
    origin = o if origin is None else np.asarray(origin, f32)
    dps = d if dps is None else f32(dps)
    t = np.array([[0.13, 0.21, 0.35], [0.81, 0.33, 0.42], [0.47, 0.92, 0.66]], np.float64) * res
    return (origin.astype(np.float64) + t * float(dps)).astype(f32).reshape(1, 9)


def dyadic_grid(verts, res):
    """an explicit grid around `verts` (n, 3): dps the smallest power of two whose res^3 grid holds them, origin a multiple of dps -- so that
    origin + k * dps is exact in float32 and lattice-coincident triangles stay lattice-coincident"""
    lo, hi = verts.min(0).astype(np.float64), verts.max(0).astype(np.float64)
    dps = 2.0 ** np.ceil(np.log2((hi - lo).max() / (res - 1)))
    origin = np.floor(lo / dps) * dps
    assert (origin + dps * res > hi).all()
    return origin.astype(f32), f32(dps)


_mixed = {}


def mixed_mesh(res=256, n_bunny=3000, n_per_class=40, span=96):
    """(tris (m, 9), origin, dps): every triangle class (span 96 voxels: footprints on both sides of the voxelizer's whole-wave threshold of 2048 cells)
    dealt one by one between 3000 bunny triangles, so lane-own and whole-wave triangles sit in the same waves"""
    key = (res, n_bunny, n_per_class, span)
    if key not in _mixed:
        bunny = bunny_tris()[:n_bunny]
        origin, dps = dyadic_grid(bunny.reshape(-1, 3), res)
        cl = triangle_classes(res, n_per_class, seed=5, span=span, origin=origin, dps=dps)
        adv = np.stack([cl[k] for k in CLASSES], 1).reshape(-1, 9)  # class after class, round robin
        step = len(bunny) // len(adv)
        parts = []
        for i in range(len(adv)):
            parts += [bunny[i * step:(i + 1) * step], adv[i:i + 1]]
        parts.append(bunny[len(adv) * step:])
        _mixed[key] = (np.concatenate(parts).astype(f32), origin, dps)
    return _mixed[key]


def vertex_attributes(n_tris, seed):
    """random colours in [0, 1), emission on a tenth of the triangles: (n, 9) float32 each"""
    rng = np.random.default_rng(seed)
    cols = rng.random((n_tris, 9)).astype(f32)
    emis = np.where(rng.random((n_tris, 1)) < 0.1, rng.random((n_tris, 9)), 0.0).astype(f32)
    return cols, emis


# ---- triangle builds on the GPU -----------------------------------------------------------------------------------------------------------------
CONSERVATIVE = 4  # MVRT_BUILD_CONSERVATIVE


def class_build_cases():
    """[(key, tris, origin, dps, res, flags)]: every class plus one generic triangle at 32^3 and 4^3, six-separating and conservative"""
    out = []
    for res in (32, 4):
        origin, dps = class_grid(res)
        cl = triangle_classes(res)
        for name in CLASSES:
            tris = np.concatenate([cl[name][:150], one_generic_triangle(res), cl[name][150:]])
            for flags in (0, CONSERVATIVE):
                out.append(("gpubuild/%s/%d/%d" % (name, res, flags), tris, origin, dps, res, flags))
    return out


def mixed_build_cases():
    tris, origin, dps = mixed_mesh()
    return [("gpubuild/mixed/256/%d" % flags, tris, origin, dps, 256, flags) for flags in (0, CONSERVATIVE)]


def reference_build(walk, tris, origin, dps, res, flags):
    """what a triangle build must give, from the compiled reference alone: [dumped count, sorted unique codes, mask, children, psum] of the
    reference's voxel list and its embedded DAG build of that list"""
    m, _ = walk.voxelize(tris, origin, dps, res, six_separating=not (flags & CONSERVATIVE))
    u = np.unique(m)
    return [np.array([len(m)], np.uint64), u] + node_fields(walk.build_octree(u, res, dag=True, embed=True))


# ---- voxel sets of the builder pins ---------------------------------------------------------------------------------------------------------------
def voxel_set(levels, n_cluster, n_scattered, seed):
    """the random voxel sets of tests/test_gpu_upload_shapes.py (random7 = (7, 20000, 2000, 7), random9 = (9, 30000, 3000, 9)): sorted unique codes"""
    rng = np.random.default_rng(seed)
    res = 1 << levels
    box = max(2, res // 3)
    pts = np.concatenate([rng.integers(0, box, (n_cluster, 3)) + res // 4, rng.integers(0, res, (n_scattered, 3))])
    return np.unique(D.morton(pts))


def builder_scenes(O):
    """{name: (sorted unique Morton codes, gridRes)}"""
    out = {}
    tris = bunny_tris()
    for res in (16, 64, 256):
        out["bunny%d" % res] = (O.build_scene_from_triangles(tris, res).morton, res)
    out["single1"] = (np.array([int(np.random.default_rng(101).integers(0, 8))], np.uint64), 2)
    out["random7"] = (voxel_set(7, 20_000, 2_000, 7), 128)
    out["random9"] = (voxel_set(9, 30_000, 3_000, 9), 512)
    out["full8"] = (np.arange(512, dtype=np.uint64), 8)
    return out


# ---- rays -----------------------------------------------------------------------------------------------------------------------------------------
def random_rays(lo, hi, n, seed):
    """tests/test_gpu_parity.py::random_rays on explicit bounds: a tenth each with a zero x / y / z component, 50 straight down, a tenth from inside"""
    rng = np.random.default_rng(seed)
    c = (lo + hi) / 2
    ext = (hi - lo).max()
    ro = (c + (rng.random((n, 3)) - 0.5) * ext * 2.5).astype(f32)
    tgt = (lo + rng.random((n, 3)) * (hi - lo)).astype(f32)
    rd = (tgt - ro).astype(f32)
    k = n // 10
    rd[:k, 0] = 0.0
    rd[k:2 * k, 1] = 0.0
    rd[2 * k:3 * k, 2] = 0.0
    rd[3 * k:3 * k + 50] = np.array([0, 0, -1], f32)
    ro[4 * k:5 * k] = (lo + rng.random((k, 3)) * (hi - lo)).astype(f32)
    return ro, rd


TIE_DIRS = [(1, 1, 1), (1, 1, -1), (1, -1, 1), (-1, 1, 1), (1, 1, 0.5), (1, 0.5, 1), (0.5, 1, 1), (1, 0.5, 0.25), (2, 1, 1), (1, 2, -1), (-1, -1, -1), (1, -1, -0.5)]


def tie_rays(lo, ext, levels, seed=3, n_out=6000, n_on=3000):
    """the rays of tests/test_gpu_parity.py::test_trace_tie_cases_bit_exact for a grid of `levels` levels: diagonals through node corners from dyadic
    distances outside (exact ties between mid-plane and exit times), and the same directions from ON the corners"""
    ext = f32(ext)
    rng = np.random.default_rng(seed)
    top = min(levels, 8)
    ros, rds = [], []
    for k in range(n_out):
        lvl = int(rng.integers(1, top + 1))
        cell = ext / f32(2 ** lvl)
        p = lo + cell * rng.integers(0, 2 ** lvl + 1, size=3).astype(f32)
        d = np.array(TIE_DIRS[k % len(TIE_DIRS)], f32)
        s = f32(2 ** int(rng.integers(0, 3)))
        ros.append((p - d * ext * s).astype(f32))
        rds.append(d if k % 3 else d * f32(0.5))
    for k in range(n_on):
        lvl = int(rng.integers(1, top + 1))
        cell = ext / f32(2 ** lvl)
        p = lo + cell * rng.integers(0, 2 ** lvl + 1, size=3).astype(f32)
        ros.append(p.astype(f32))
        rds.append(np.array(TIE_DIRS[k % len(TIE_DIRS)], f32))
    return np.array(ros, f32), np.array(rds, f32)


def on_voxel_rays(lo, dps, morton, n, seed):
    """origins ON voxels of the scene -- corners, edge midpoints and face centres in turn -- with random directions, a quarter along a TIE_DIRS diagonal"""
    rng = np.random.default_rng(seed)
    cells = D.decode(morton[rng.integers(0, len(morton), n)]).astype(f32)
    off = rng.integers(0, 2, (n, 3)).astype(f32)
    halves = np.arange(n) % 3  # 0: corner, 1: edge midpoint, 2: face centre
    for h in (1, 2):
        rows = np.flatnonzero(halves == h)
        for j in range(h):
            off[rows, (rows + j) % 3] = 0.5
    ro = (lo + f32(dps) * (cells + off)).astype(f32)
    rd = rng.normal(size=(n, 3)).astype(f32)
    rd[::4] = np.array(TIE_DIRS, f32)[np.arange(len(rd[::4])) % len(TIE_DIRS)]
    return ro, rd


SPECIAL = np.array([0.0, -0.0, 1e-45, -1e-40, 1.1754942e-38, 1e38, -3.4028235e38, np.inf, -np.inf, np.nan], np.float32)


def special_direction_rays(ro, rd, n, seed):
    """the first n of (ro, rd) with one, two or all three direction components replaced by +-0, denormals, the largest denormal, huge values,
    +-inf and NaN"""
    rng = np.random.default_rng(seed)
    ro, rd = ro[:n].copy(), rd[:n].copy()
    for i in range(len(rd)):
        axes = rng.permutation(3)[: 1 + i % 3]
        rd[i, axes] = SPECIAL[rng.integers(0, len(SPECIAL), len(axes))]
    return ro, rd


class RayScene:
    """what a traversal pin needs of a scene: embedded nodes (root last), bounds as the oracle computes them, grid, sorted codes"""

    def __init__(self, name, sc, levels, deep=None):
        self.name, self.sc, self.levels, self.deep = name, sc, levels, deep
        self.nodes = sc.nodes
        self.lower, self.upper = sc.bounds()
        self.dps, self.morton = f32(sc.dps), sc.morton
        assert len(self.nodes) < 0xFFFFFF and levels <= 32


def ray_set(rs, n_random=100_000):
    """(ro, rd, isShadow) of a RayScene: n_random mixed rays (zero components, from inside), the tie rays, origins on voxel corners / edges / faces,
    secondary-style origins ro + rd * t of the oracle's own hits, special direction components; deep scenes add their aimed short, long and tie rays.
    Every third ray is a shadow ray."""
    lo, hi = rs.lower, rs.upper
    parts = [random_rays(lo, hi, n_random, 7), tie_rays(lo, (hi - lo).max(), rs.levels), on_voxel_rays(lo, rs.dps, rs.morton, 6000, 11)]
    if rs.deep is not None:
        ro, rd, _, _ = rs.deep.short_rays(3000, 21)
        parts += [(ro, rd), rs.deep.long_rays(3000, 22), rs.deep.tie_rays(3000, 23)]
    ro, rd = (np.concatenate([p[k] for p in parts]) for k in (0, 1))
    first = rs.sc.trace(ro, rd, threads=8)
    hit = first["t"] != MAXF
    rng = np.random.default_rng(13)
    ro2 = (ro[hit] + rd[hit] * first["t"][hit][:, None]).astype(f32)[:20_000]
    rd2 = rng.normal(size=ro2.shape).astype(f32)
    ro3, rd3 = special_direction_rays(ro, rd, 6000, 17)
    ro4, rd4 = special_direction_rays(ro2, rd2, 3000, 19)
    ro = np.concatenate([ro, ro2, ro3, ro4])
    rd = np.concatenate([rd, rd2, rd3, rd4])
    return ro, rd, (np.arange(len(ro)) % 3 == 0).astype(np.uint8)


_ray_scenes = {}


def ray_scene(O, name):
    """bunny16 ... bunny1024, random7, random9, deep14 ... deep21"""
    if name not in _ray_scenes:
        if name.startswith("bunny"):
            res = int(name[5:])
            rs = RayScene(name, O.build_scene_from_triangles(bunny_tris(), res), res.bit_length() - 1)
        elif name.startswith("random"):
            levels = int(name[6:])
            m = voxel_set(levels, *{7: (20_000, 2_000, 7), 9: (30_000, 3_000, 9)}[levels])
            res = 1 << levels
            sc = O.Scene(O.build_octree(m, res), np.zeros((len(m), 8), np.uint8), np.zeros(3, f32), f32(1.0 / res), res)
            sc.morton = m
            rs = RayScene(name, sc, levels)
        else:
            s = D.scene(int(name[4:]))
            rs = RayScene(name, D.oracle_scene(O, s), s.levels, deep=s)
        _ray_scenes[name] = rs
    return _ray_scenes[name]


RAY_SCENES = ["bunny16", "bunny64", "bunny256", "bunny1024", "random7", "random9"] + ["deep%d" % L for L in D.DEPTHS]
_ray_sets = {}


def rays_of(O, name):
    if name not in _ray_sets:
        _ray_sets[name] = ray_set(ray_scene(O, name))
    return _ray_sets[name]
