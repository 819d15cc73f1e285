"""The revisit of a popped node (csrc/traverse_stream.h): the flavours that keep the voxel path take the resume point -- the candidate the node
was left through -- from the path and FILTER the recomputed candidate chain with it; stack entries hold the plain exit times.  The smallest
shapes at which that can go wrong, each against the CPU oracle element for element (t, nMajor, vIndex, descents; frame buffer and counters
for the path tracer):
  * every mirror mask (the resume point is a MIRRORED child index, the path holds real ones),
  * ancestors stacked by the hint replay (their resume point comes from the hint's prefix),
  * more pending ancestors than the LDS ring has slots (evicted entries come back from the HBM spill rows in the same format),
  * tied mid-plane times (candidates of the chain coincide: the filter must not admit the child already taken again)."""

import numpy as np
import pytest

import deep_scenes as D
from common import bunny_tris, hdr_bytes, position_colors, probe_camera
from fixtures import mv, O  # noqa: F401 (fixtures)
from rays import assert_hits_equal, voxel_scene

pytestmark = pytest.mark.gpu

MAXF = np.float32(3.402823466e38)
FLAGS = [0, 2, 3]  # embedded masks / plain indices / tree (bricks): flavours 0, 1, 2


def build(mv, s, flags):
    svo = mv.IntersectorOctreeGPU()
    svo.build_voxels(s.xyz, s.attrs, origin=s.origin, dps=s.dps, gridRes=s.res, flags=flags)
    assert svo.info().flavour == (2 if flags == 3 else int(flags == 2))
    return svo


# ---- all mirror combinations ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sparse64():
    rng = np.random.default_rng(640)
    s = voxel_scene(rng.integers(0, 64, size=(5300, 3)), 64)  # ~2 % of 64^3
    n = 8192
    ro = rng.random((n, 3)).astype(np.float32)  # inside the grid (the unit cube)
    mag = (0.05 + rng.random((n, 3))).astype(np.float32)
    k = np.arange(n) % 8
    sign = np.stack([np.where(k & 1, -1.0, 1.0), np.where(k & 2, -1.0, 1.0), np.where(k & 4, -1.0, 1.0)], -1).astype(np.float32)
    sh = (np.arange(n) % 5 == 0).astype(np.uint8)
    return s, ro, (mag * sign).astype(np.float32), sh, k


@pytest.mark.parametrize("flags", FLAGS)
def test_all_mirror_masks(mv, O, sparse64, flags):
    s, ro, rd, sh, k = sparse64
    sc = D.oracle_scene(O, s, flags)
    want = sc.trace(ro, rd, sh, threads=8, want_descents=True)
    # Pops, from the oracle's descent counts.  A descent that is not on the path to the hit voxel is undone by a pop, and one pop undoes at most `levels`
    # of them (leaf level back to the root), so a ray that hits after W wasted descents has popped at least W / levels times: twice if W > levels.  A ray
    # that misses ends with a pop from the empty stack, which resumes nothing: one chain of wasted descents more, twice if W > 2 * levels.
    levels = 6
    hit = want["t"] != MAXF
    wasted = want["descents"].astype(np.int64) - np.where(hit, levels, 0)
    popped_twice = np.where(hit, wasted > levels, wasted > 2 * levels)
    print("rays that pop at least twice: %.3f, hits %.3f, mean descents %.1f" % (popped_twice.mean(), hit.mean(), want["descents"].mean()))
    assert popped_twice.mean() >= 1.0 / 3.0
    for m in range(8):  # every mirror mask on its own
        assert popped_twice[k == m].sum() > 200, m
    assert_hits_equal(want, build(mv, s, flags).intersect(ro, rd, sh, want_descents=True))


# ---- replayed ancestors -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bunny_frame(O):
    tris = bunny_tris()
    cols, emis = position_colors(tris)
    sc = O.build_scene_from_triangles(tris, 256, cols, emis)
    rgba, hw, hh = O.decode_rgbe(hdr_bytes())
    w, h = 64, 36
    cam = probe_camera(sc.origin, sc.dps, 256, focus=9.0, lens_r=0.05)
    fb, _, cnt = sc.render_pt(O.HDRI(rgba, hw, hh, rgba, hw, hh, math_mode=1), cam, w, h, 0, math_mode=1, threads=8)
    return sc, (rgba, hw, hh), cam, w, h, fb, cnt


@pytest.mark.parametrize("hints", [True, False])
def test_path_tracer_step_with_and_without_hints(mv, bunny_frame, hints):
    sc, (rgba, hw, hh), cam, w, h, fb, cnt = bunny_frame
    pt = mv.PathTracer()
    pt.setup(None)
    pt.resizeFrameBufferIfNeeded(None, w, h)
    pt.loadHDRIPixels(None, rgba, hw, hh, rgba, hw, hh)
    pt.set_origin_hints(hints)
    pt.m_intersectorOctreeGPU.upload(sc.nodes, sc.attrs, sc.origin, sc.dps, sc.grid_res, sc.has_emission)
    pt.step(None, cam)
    assert np.array_equal(pt.read_framebuffer()[: w * h], fb)
    st = pt.stats()
    for key in ("rays", "descents", "shadowDescents", "hits"):
        assert st[key] == cnt[key], key


# ---- deep stack ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plate1024():
    """A one-voxel-thick plate y = 300 over the whole x range of a 1024^3 grid (10 levels), 256 voxels wide in z, and rays that skim along x in the
    voxel row right above it (y = 301: the same cell as the plate at every level above the voxels, 300 being even) from inside the first voxel
    column, dropping one voxel in 300 to 900.  At every level from the root to the grandparents of voxels the ray is in the first half of a node
    whose second half holds plate voxels as well: a later valid candidate, so the node is stacked -- levels 0 to 8, nine pending ancestors, more
    than the 8 slots of the embedded flavour's ring (the push at level 8 evicts the root's entry to the spill rows) and more than twice the 4
    slots of the plain-index flavour's.  The parents of voxels along the ray hold no voxel in its row, so the walk pops its way along x, the evicted
    entries included, until the ray reaches the plate.  Both directions of travel, and a quarter of the rays along z instead (the plate is 256
    voxels wide there: they stack fewer levels, and many leave the plate before they reach it)."""
    res, H = 1024, 300
    x, z = np.meshgrid(np.arange(res), np.arange(384, 640), indexing="ij")
    s = voxel_scene(np.stack([x.ravel(), np.full(x.size, H), z.ravel()], -1), res)
    rng = np.random.default_rng(1024)
    n = 4096
    i = np.arange(n)
    back, swap = i % 2 == 1, (i // 2) % 4 == 3              # travel in the negative direction; along z instead of x
    lo, hi = np.where(swap, 384.0, 0.0), np.where(swap, 640.0, 1024.0)
    inset = 0.05 + 0.9 * rng.random(n)                      # voxel units: inside the first voxel column of the plate
    a = np.where(back, hi - inset, lo + inset)              # coordinate along the travel axis
    c = np.where(swap, 16.0 + 992.0 * rng.random(n), 400.0 + 224.0 * rng.random(n))  # across it: on the plate, with room for the drift
    y = H + 1.05 + 0.9 * rng.random(n)                      # the voxel row above the plate
    da = np.where(back, -1.0, 1.0)
    dy = -1.0 / (300.0 + 600.0 * rng.random(n))
    dc = (rng.random(n) - 0.5) * 0.02
    ro = np.where(swap[:, None], np.stack([c, y, a], -1), np.stack([a, y, c], -1)) / res
    rd = np.where(swap[:, None], np.stack([dc, dy, da], -1), np.stack([da, dy, dc], -1))
    sh = (i % 7 == 0).astype(np.uint8)
    return s, ro.astype(np.float32), rd.astype(np.float32), sh, swap


@pytest.mark.parametrize("flags", FLAGS)
def test_more_pending_ancestors_than_ring_slots(mv, O, plate1024, flags):
    s, ro, rd, sh, swap = plate1024
    sc = D.oracle_scene(O, s, flags)
    want = sc.trace(ro, rd, sh, threads=8, want_descents=True)
    hit = want["t"] != MAXF
    print("hits %.3f, mean descents %.1f (along x %.1f)" % (hit.mean(), want["descents"].mean(), want["descents"][~swap].mean()))
    assert hit[~swap].mean() > 0.9
    # a ray along x drops 0.05 to 0.95 voxels at one in 300 to 900 before it reaches the plate: about 300 voxels of travel in the median, past a dead-end parent of
    # voxels every second voxel, each of them entered (one descent) and popped from
    assert np.median(want["descents"][~swap]) > 150
    assert_hits_equal(want, build(mv, s, flags).intersect(ro, rd, sh, want_descents=True))


# ---- filter edge: tied mid-plane times -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checker32():
    res = 32
    g = np.stack(np.meshgrid(np.arange(res), np.arange(res), np.arange(res), indexing="ij"), -1).reshape(-1, 3)
    s = voxel_scene(g[g.sum(1) % 2 == 0], res)
    rng = np.random.default_rng(32)
    dirs = []
    for ax in range(3):                                      # axis-parallel
        for sg in (1.0, -1.0):
            d = np.zeros(3)
            d[ax] = sg
            dirs.append(d)
    for sx in (1.0, -1.0):                                   # exactly diagonal: space diagonals, face diagonals, and the partial ties of test_degenerate_octrees
        for sy in (1.0, -1.0):
            dirs += [np.array([sx, sy, 1.0]), np.array([sx, sy, -1.0]), np.array([sx, sy, 0.0]), np.array([sx, 0.0, sy]), np.array([0.0, sx, sy])]
    dirs += [np.array(d) for d in ((1, 1, 0.5), (-1, 1, 0.5), (0.5, 1, -1), (1, 0.5, 0.25), (-2, 1, 1), (1, -2, -1))]
    dirs = np.array(dirs, np.float32)
    n = 6000
    d = dirs[np.arange(n) % len(dirs)]
    # through lattice points, cell centres and edge midpoints (multiples of half a cell): mid-plane times of several axes coincide at every level
    p = (rng.integers(0, 2 * res + 1, size=(n, 3)) / np.float32(2 * res)).astype(np.float32)
    kind = (np.arange(n) // len(dirs)) % 3
    step = np.where(kind == 0, 2.0, np.where(kind == 1, 0.25, 0.0)).astype(np.float32)  # from outside the grid, from a dyadic distance inside it, from ON the point
    ro = (p - d * step[:, None]).astype(np.float32)
    sh = (np.arange(n) % 4 == 0).astype(np.uint8)
    return s, ro, d.copy(), sh


@pytest.mark.parametrize("flags", FLAGS)
def test_tied_candidates(mv, O, checker32, flags):
    s, ro, rd, sh = checker32
    sc = D.oracle_scene(O, s, flags)
    want = sc.trace(ro, rd, sh, threads=8, want_descents=True)
    hit = want["t"] != MAXF
    print("hits %.3f, rays with descents beyond the hit's path %.3f" % (hit.mean(), (want["descents"] > np.where(hit, 5, 0)).mean()))
    assert 0.2 < hit.mean() and (want["descents"][hit] > 5).mean() > 0.2  # hits, and a good share of them after dead ends (pops)
    assert_hits_equal(want, build(mv, s, flags).intersect(ro, rd, sh, want_descents=True))
