"""Inputs, fixtures and the comparison rule of the pins against the COMPILED reference (oracle/_ref/libmvrt_ref_walk.so, built by `make -C oracle ref`
from voxCommon.hpp, voxelization.hpp, morton.hpp and IntersectorOctree.hpp as they lie, and libmvrt_ref_render.so, from the host branch of
renderCommon.hpp and pmjSampler.hpp): tests/test_reference_pins_cpu.py (oracle == reference) and
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
    """the random voxel sets of tests/upload_shapes.py (random7 = (7, 20000, 2000, 7), random9 = (9, 30000, 3000, 9)): sorted unique codes"""
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
    """tests/rays.py::random_rays on explicit bounds: a tenth each with a zero x / y / z component, 50 straight down, a tenth from inside"""
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


FAR_K = 24  # origins extent * 2^k away, k = 0 .. 23: at k = 23 one float32 rounding of an origin coordinate or of a slab time spans the whole grid
FAR_SCENES = ("bunny64", "deep16", "deep21")  # the far-ray pins against the compiled reference: 16 levels is the device view's limit, 21 the library's
N_FAR_PIN = 60_000


def far_rays(rs, n, seed):
    """(ro, rd, isShadow, k) of a RayScene: n rays at a random point of a random voxel from an origin extent * 2^k away, k uniform in 0 .. 23.  A third of
    the directions are flattened by 1e-3 on one axis (grazing rays).  The direction is taken from the origin as float32 holds it and scaled by
    2^-20 .. 2^20, so t covers 2^-20 .. 2^43 extents.  Not part of ray_set: the digests of the trace/ keys do not contain these rays.  Every third ray
    is a shadow ray."""
    rng = np.random.default_rng(seed)
    lo, ext = rs.lower.astype(np.float64), float((rs.upper - rs.lower).max())
    cells = D.decode(rs.morton[rng.integers(0, len(rs.morton), n)]).astype(np.float64)
    tgt = lo + float(rs.dps) * (cells + rng.random((n, 3)))
    u = rng.normal(size=(n, 3))
    flat = np.flatnonzero(np.arange(n) % 3 == 1)
    u[flat, rng.integers(0, 3, len(flat))] *= 1e-3
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    k = rng.integers(0, FAR_K, n)
    ro = (tgt - u * (ext * 2.0 ** k)[:, None]).astype(f32)
    d = tgt - ro.astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rd = (d * (2.0 ** rng.integers(-20, 21, n))[:, None]).astype(f32)
    return ro, rd, (np.arange(n) % 3 == 0).astype(np.uint8), k.astype(np.int32)


_far_sets = {}


def far_rays_of(O, name, n, seed=29):
    if (name, n, seed) not in _far_sets:
        _far_sets[(name, n, seed)] = far_rays(ray_scene(O, name), n, seed)
    return _far_sets[(name, n, seed)]


# ---- the renderer's sampling code: oracle/_ref/libmvrt_ref_render.so ------------------------------------------------------------------------------
BELOW1 = np.nextafter(f32(1), f32(0))  # the largest float below 1


def load_render(O, tree_decides):
    """the RefRender of oracle/_ref, or None; the rules of load_walk"""
    ref = O.load_ref()
    if tree_decides and os.path.isdir(REFERENCE_TREE):
        assert ref is not None and ref.render is not None, "the reference tree is present but oracle/_ref is not built: run __graft_entry__.build() (make -C oracle ref)"
    if ref is None:
        return None
    assert ref.render is not None, "oracle/_ref holds libmvrt_ref.so but not libmvrt_ref_render.so: rebuild it (make -C oracle ref)"
    return ref.render


def needs_libm(render, what):
    """answers that pass through sinf / cosf / atan2f / powf depend on the host's C library: no digest is stored for them, and without the compiled
    reference they skip by name"""
    if render is None:
        import pytest
        pytest.skip(what + ": depends on the host's libm, compared only where oracle/_ref/libmvrt_ref_render.so is present")


def cameras():
    """{name: 15 floats}.  probe: an orthonormal look-at with a lens.  skew: a rotated basis that is neither orthogonal nor of unit length, with odd
    values everywhere -- no product in shoot / shootThinLens is exact, so every association of the reference's expressions shows in the last bit."""
    from common import probe_camera
    rng = np.random.default_rng(71)
    skew = np.zeros(15, f32)
    skew[0:3] = (-3.7, 2.9, 11.3)
    skew[3:12] = (rng.normal(size=9) * [1, 1, 1, 0.7, 0.7, 0.7, 1.3, 1.3, 1.3]).astype(f32)
    skew[12], skew[13], skew[14] = f32(0.41421357), f32(0.037), f32(7.3)
    return {"probe": probe_camera(np.zeros(3, f32), f32(1 / 64), 64, focus=9.0, lens_r=0.05), "skew": skew}


CAMERA_SIZES = [(97, 61), (64, 40), (1, 1), (7, 5), (1920, 1080), (61, 97)]


def camera_rays(n_random=400, seed=72):
    """(px (n, 4) int32 x, y, W, H; fl (n, 4) float32 xo, yo, u0, u1): per image size, the four corner pixels with every combination of pixel offset and
    lens sample in {0, the float below 1}, then random pixels with random offsets, a quarter of them with one offset / lens sample at an end"""
    rng = np.random.default_rng(seed)
    px, fl = [], []
    ends = np.array([[a, b, c, d] for a in (0, BELOW1) for b in (0, BELOW1) for c in (0, BELOW1) for d in (0, BELOW1)], f32)
    for W, H in CAMERA_SIZES:
        for x in sorted({0, W - 1}):
            for y in sorted({0, H - 1}):
                px.append(np.tile(np.array([x, y, W, H], np.int32), (16, 1)))
                fl.append(ends)
        p = np.stack([rng.integers(0, W, n_random), rng.integers(0, H, n_random), np.full(n_random, W), np.full(n_random, H)], 1).astype(np.int32)
        f = rng.random((n_random, 4), dtype=f32)
        k = n_random // 4
        f[np.arange(k), rng.integers(0, 4, k)] = np.where(rng.random(k) < 0.5, f32(0), BELOW1)
        px.append(p)
        fl.append(f)
    return np.concatenate(px), np.concatenate(fl)


def unit_normals(n, seed):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)


DENORMAL = f32(1e-45)
SPECIAL_NORMALS = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, 0, -0.0], [1, 0, -0.0], [1, 0, DENORMAL], [0, 1, -DENORMAL],
                            [0.6, 0.8, DENORMAL], [0.6, -0.8, -0.0], [0.6, 0, -0.8], [0, -0.6, 0.8]], f32)


def lambert_inputs(n_random=20_000, seed=73):
    """(ab (n, 2), normals (n, 3)): the special normals (both signs of every axis, z = -1 exactly, z = -0 and z a denormal of either sign) with a in
    {0, 1, random} and b in {0, the float below 1, random}; then random unit normals with random a, b"""
    rng = np.random.default_rng(seed)
    ab = np.array([[a, b] for a in (0, 1, 0.37, BELOW1) for b in (0, BELOW1, 0.25, 0.5, 0.61)], f32)
    n = np.repeat(SPECIAL_NORMALS, len(ab), 0)
    ab = np.tile(ab, (len(SPECIAL_NORMALS), 1))
    return np.concatenate([ab, rng.random((n_random, 2), dtype=f32)]), np.concatenate([n, unit_normals(n_random, seed + 1)])


PT_DIMENSIONS = 28  # kPtGenerate uses dimensions 0 (pixel jitter) and 1 (lens); the shade kernel 2 .. 27: per bounce two for the light sample, one for the
#                     bounce, at the first bounce one more for the extra direct sample (oracle/mvrt_oracle.cpp ptSample): 2 + 1 + 8 * 3 = 27 drawn at most


def sample2d_inputs():
    """(sampleIdx, dimension, stream) uint32 (n,): sample indices 0 .. 4095 and beyond the table's length, every dimension the path tracer draws and
    dimensions beyond the 128 sequences, streams 0, 2^32 - 1 and two in between -- the full product"""
    idx = np.concatenate([np.arange(4096), [4096, 4097, 8191, 65536, 2**31, 2**32 - 1]]).astype(np.uint32)
    dim = np.concatenate([np.arange(PT_DIMENSIONS + 4), [127, 128, 129, 2**32 - 1]]).astype(np.uint32)
    stream = np.array([0, 2**32 - 1, 0x9E3779B9, 1], np.uint32)
    g = np.meshgrid(idx, dim, stream, indexing="ij")
    return tuple(np.ascontiguousarray(a.reshape(-1)) for a in g)


def hdri_map(name):
    """(rgba, w, h) of the maps of tests/hdri_maps.py that the importance-sampling pins use"""
    import hdri_maps as M
    if name.startswith("noise"):
        w, h = (int(v) for v in name[5:].split("x"))
        return M.noise(w, h, seed=w * 1000 + h), w, h
    return {"sun": lambda: (M.sun(520, 260), 520, 260), "black_ground": lambda: (M.black_ground(64, 32), 64, 32),
            "denormal_floor": lambda: (M.denormal_floor(64, 32), 64, 32), "all_black": lambda: (M.all_black(8, 4), 8, 4)}[name]()


HDRI_MAPS = ["noise1x1", "noise2x1", "noise1x2", "noise7x5", "noise64x32", "noise520x260", "sun", "black_ground", "denormal_floor"]
K08 = f32(0.8)
# normals on both sides of importanceSample's 0.8 threshold on every axis, exactly 0.8 included (k < N.x is false there: the next test decides), then
# normals that select the uniform table
HDRI_NORMALS = np.array([[s * v if a == 0 else 0, s * v if a == 1 else 0, s * v if a == 2 else 0] for a in range(3) for s in (1, -1)
                         for v in (f32(1), np.nextafter(K08, f32(1)), K08, np.nextafter(K08, f32(0)))] + [[0.8, 0.9, 0], [-0.8, -0.8, -0.9], [0.5, 0.5, 0.70710678]], f32)


def table_of_normal(n):
    """which of the seven tables (0 uniform, 1 .. 6 = +x, -x, +y, -y, +z, -z) importanceSample( axisAligned ) takes for the normals n (k, 3): the chain of
    renderCommon.hpp:371-398, restated on integers for the tests' bookkeeping only (which cases have a total); the compared values never pass through it"""
    n = np.asarray(n, f32)
    out = np.zeros(len(n), np.int32)
    for which, (axis, positive) in reversed(list(enumerate([(0, True), (0, False), (1, True), (1, False), (2, True), (2, False)], 1))):
        sel = (K08 < n[:, axis]) if positive else (n[:, axis] < -K08)
        out[sel] = which
    return out


def hdri_inputs(tables7, w, h, n_random=1500, seed=74):
    """(N (k, 3), u (k, 4)): for each normal of HDRI_NORMALS -- u0 / u1 at 0, at the float below 1 and ON entries of the table that the normal selects
    (prefix / 0xFFFFFFFF rounded to float, where `value <= b` decides between two texels), u2 / u3 at 0 and below 1, then random u"""
    rng = np.random.default_rng(seed)
    which = table_of_normal(HDRI_NORMALS)
    Ns, us = [], []
    for N, t in zip(HDRI_NORMALS, which):
        tab = np.asarray(tables7[t], np.uint32).reshape(h, w)
        ends = [[a, b, c, d] for a in (0, BELOW1) for b in (0, BELOW1) for c in (0, BELOW1) for d in (0, BELOW1)]
        row = tab[h - 1].astype(np.float64)
        on_h = (row[rng.integers(0, w, 12)] .astype(f32) / f32(0xFFFFFFFF)).astype(f32)
        on_h = on_h[on_h < 1]
        on = [[v, rng.random(), rng.random(), rng.random()] for v in on_h] + [[np.nextafter(v, f32(0)), rng.random(), rng.random(), rng.random()] for v in on_h]
        # u1 on an entry of the chosen column: V( X, y ) / vol as the reference forms it, for a few columns; u0 = the column's own start selects it
        for x in rng.integers(0, w, 6):
            lo = 0 if x == 0 else int(tab[h - 1, x - 1])
            vol = (int(tab[h - 1, x]) - lo) & 0xFFFFFFFF
            if vol == 0:
                continue
            u0 = f32(f32(lo) / f32(0xFFFFFFFF))
            y = int(rng.integers(0, h))
            v = (int(tab[y, x]) - (0 if x == 0 else int(tab[y, x - 1]))) & 0xFFFFFFFF
            u1 = f32(f32(v) / f32(vol))
            if u0 < 1 and u1 < 1:
                on += [[u0, u1, rng.random(), rng.random()], [u0, np.nextafter(u1, f32(0)), rng.random(), rng.random()]]
        u = np.concatenate([np.array(ends, f32), np.array(on, f32).reshape(-1, 4), rng.random((n_random // len(HDRI_NORMALS), 4), dtype=f32)])
        Ns.append(np.tile(N, (len(u), 1)))
        us.append(u)
    return np.concatenate(Ns), np.concatenate(us)


# ---- frames composed from the compiled reference alone (tests/test_gpu_reference_pins.py) ---------------------------------------------------------
class ReferenceProvider:
    """the provider of tests/aov_expected.py over the compiled reference: PMJSampler::sample2d on PMJSampler::setup's own table and
    CameraPinhole::shootThinLens from the render library, octreeTraverse_EfficientParametric from the walk library"""

    def __init__(self, render, walk):
        self.render, self.walk = render, walk

    def sample2d(self, sample_idx, dim, stream):
        return self.render.sample2d(self.render.pmj_table(), sample_idx, dim, stream)

    def shoot_thin_lens(self, cam, px, fl):
        return self.render.camera_shoot(cam, px, fl, True)

    def trace(self, sc, ro, rd):
        lower, upper = sc.bounds()
        return self.walk.trace(sc.nodes, lower, upper, ro, rd)


_frame_scene = None


def frame_scene(O):
    """bunny at 64^3 with colours (the octree itself is pinned to the reference's builder by test_builder)"""
    global _frame_scene
    if _frame_scene is None:
        from common import position_colors
        tris = bunny_tris()
        cols, emis = position_colors(tris)
        _frame_scene = O.build_scene_from_triangles(tris, 64, cols, emis)
    return _frame_scene


def frame_cameras(sc):
    """{name: 15 floats}, lensR 0.05: `outside` looks at the grid from far off (the probe camera), `inside` stands in the grid's upper corner region, within the
    bounds, and looks across the model -- its rays start inside the root node"""
    from common import probe_camera
    ext = float(sc.dps) * sc.grid_res
    return {"outside": probe_camera(sc.origin, sc.dps, sc.grid_res, focus=9.0, lens_r=0.05),
            "inside": probe_camera(sc.origin, sc.dps, sc.grid_res, focus=0.5 * ext, lens_r=0.05, offset=(0.42 * ext, 0.38 * ext, 0.45 * ext))}


PRIMARY_SIZES = [(97, 61), (64, 40)]


def reference_primary(pair, sc, cam, W, H):
    """the `render` kernel's rays composed from the reference: CameraPinhole::shoot through every pixel centre (voxKernel.cu:437-483 passes 0.5f, 0.5f), then
    octreeTraverse_EfficientParametric -> [t, nMajor, vIndex]; a miss keeps MAX_FLOAT, -1, 0"""
    render, walk = pair
    p = np.arange(W * H)
    px = np.stack([p % W, p // W, np.full(W * H, W), np.full(W * H, H)], 1).astype(np.int32)
    fl = np.tile(np.array([0.5, 0.5, 0, 0], f32), (W * H, 1))
    ro, rd = render.camera_shoot(cam, px, fl, False)
    lower, upper = sc.bounds()
    return list(walk.trace(sc.nodes, lower, upper, ro, rd).values())


FIRST_HIT_SIZE = (64, 40)


def reference_first_hit(pair, O, sc, cam):
    """[normal/depth buffer (W * H, 4)] of one 16-spp step at 64x40 with the sampler, the thin-lens camera and the traversal of the compiled reference.
    The buffer is no output of the reference (it has no such buffer): xyz is the sum of the first hits' axis normals and w the sum of their t, 16 sequential
    float32 additions per pixel in ascending sample order from +0 (include/mvrt.h) -- that derivation is restated once, in tests/aov_expected.py."""
    import aov_expected as A
    exp = A.Expected(O, sc, *FIRST_HIT_SIZE, provider=ReferenceProvider(*pair))
    exp.step(cam)
    return [exp.normal_depth]
