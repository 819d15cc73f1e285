"""The oracle's walk on octrees of 14 to 21 levels against an independent float64 walk (no GPU).

The oracle traverses in fp32 from the root's slab times down, so at 21 levels a voxel is only a few ulps of the root's t range wide.  A
vectorised Amanatides-Woo DDA in float64 over the occupied set (np.searchsorted on the sorted Morton codes) follows the reference's rule --
the first voxel whose entry t is > 0 counts, a voxel that contains the origin does not -- and decides which hits are unambiguous: the
float64 entry is farther from every other event of the walk (the other axes' plane crossings, the voxel's exit, the origin) than the fp32
t values of the two events can be off by.  The walk derives an axis' plane times from that axis' root slab times only, so they are off by
m_a = 2 ulp32(max |t| of the root slab of axis a).  Where the hit is unambiguous the oracle must give the float64 voxel, its entry axis and
t within m_a; elsewhere a voxel within one voxel (Chebyshev) of it; a ray that misses every voxel by more than the largest m_a must miss."""
import numpy as np
import pytest

import deep_scenes as D
from fixtures import O  # noqa: F401 (fixtures)

MAXF = np.float32(3.402823466e38)
N_RAYS = 9000
DDA_STEPS = 64  # short rays start at most ~9 voxels from their target: it lies within 3 * 9 cell crossings

# unambiguous share of the short rays with general directions that hit, per depth: measured (seeded) -> asserted floor
UNAMBIGUOUS_GENERAL = {14: (0.991, 0.95), 15: (0.984, 0.93), 16: (0.965, 0.90), 17: (0.940, 0.85), 20: (0.524, 0.40), 21: (0.259, 0.15)}


def ulp32(x):
    x = np.abs(np.asarray(x, np.float32))
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


def root_slab_margin(s, ro, rd):
    """m_a in t units, (n, 3): 2 ulp32 of the largest |t| of the root's slab of each axis the ray moves along (0 where it does not: no
    plane of that axis is ever crossed, its clamped t values stay near +-MAX_FLOAT)"""
    lo = s.origin.astype(np.float64)
    hi = lo + float(s.dps) * s.res
    o = ro.astype(np.float64)
    d = rd.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ta, tb = (lo - o) / d, (hi - o) / d
        return np.where(d != 0, 2.0 * ulp32(np.where(d != 0, np.maximum(np.abs(ta), np.abs(tb)), 0.0)), 0.0)


def dda(s, ro, rd, m_t, steps=DDA_STEPS):
    """float64 walk over the occupied cells for `steps` cell crossings.  Returns per ray: hit (bool), cell (n, 3), t (entry), axis (entry axis),
    clear (every event up to and including the hit is farther from every other than m_a + m_b of the two events' axes: the entry point is
    away from the face's edges, the exit, the previous crossing and the origin), graze (the hit voxel's exit is within that margin of its
    entry: the ray clips an edge or a corner of it)"""
    n = len(ro)
    p0 = s.to_voxel(ro)
    d = rd.astype(np.float64) / float(s.dps)  # voxel units per unit of t
    cell = np.floor(p0).astype(np.int64)
    step = np.sign(d).astype(np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        nxt = np.where(d > 0, cell + 1 - p0, cell - p0) / d
        delta = np.abs(1.0 / d)
    nxt = np.where(d != 0, nxt, np.inf)
    delta = np.where(d != 0, delta, np.inf)
    hit = np.zeros(n, bool)
    clear = np.ones(n, bool)
    graze = np.zeros(n, bool)
    t_hit = np.full(n, np.inf)
    axis_hit = np.full(n, -1)
    cell_hit = np.zeros((n, 3), np.int64)
    rows = np.arange(n)
    prev_t, prev_m = np.full(n, -np.inf), np.zeros(n)
    for _ in range(steps):
        live = ~hit
        if not live.any():
            break
        order = np.argsort(nxt, axis=1)
        a, b = order[:, 0], order[:, 1]
        t_in, ma = nxt[rows, a], m_t[rows, a]
        # the other axes' next crossings (the entry point's distance from the face's edges), the origin, the previous crossing
        near = (nxt[rows, b] - t_in <= ma + m_t[rows, b]) | (np.abs(t_in) <= ma) | (t_in - prev_t <= ma + prev_m)
        clear &= ~(live & near)
        cell[rows, a] += step[rows, a]
        nxt[rows, a] += delta[rows, a]
        occ = s.occupied(cell) & (t_in > 0) & live
        c = nxt.argmin(1)
        clip = occ & (nxt[rows, c] - t_in <= ma + m_t[rows, c])  # the exit: the ray may clip the voxel's edge or corner only
        clear &= ~clip
        graze |= clip
        hit |= occ
        t_hit[occ], axis_hit[occ], cell_hit[occ] = t_in[occ], a[occ], cell[occ]
        prev_t, prev_m = np.where(live, t_in, prev_t), np.where(live, ma, prev_m)
    return hit, cell_hit, t_hit, axis_hit, clear, graze


def misses_by_more_than(s, ro, rd, m_vox):
    """brute force: the ray meets no voxel's box grown by m_vox voxels at a positive exit t (float64, voxel units)"""
    vox = D.decode(s.morton).astype(np.float64)
    p0 = s.to_voxel(ro)
    d = rd.astype(np.float64) / float(s.dps)
    out = np.ones(len(ro), bool)
    for i in range(len(ro)):
        lo, hi = vox - m_vox[i], vox + 1 + m_vox[i]
        with np.errstate(divide="ignore", invalid="ignore"):
            ta, tb = (lo - p0[i]) / d[i], (hi - p0[i]) / d[i]
        inside = (p0[i] >= lo) & (p0[i] <= hi)
        t0 = np.where(d[i] != 0, np.minimum(ta, tb), np.where(inside, -np.inf, np.inf))
        t1 = np.where(d[i] != 0, np.maximum(ta, tb), np.where(inside, np.inf, -np.inf))
        tin, tout = t0.max(1), t1.min(1)
        out[i] = not ((tin <= tout) & (tout > 0)).any()
    return out


def test_numpy_morton_codes_are_the_oracles(O):
    """the walk's occupancy lookups use their own encoder: it must give the oracle's codes, bit 62 included"""
    s = D.scene(21)
    xyz = np.concatenate([s.xyz, np.array([[0, 0, 0], [(1 << 21) - 1] * 3, [1 << 20, 0, 0], [0, 0, 1 << 20]], np.uint32)])
    assert np.array_equal(D.morton(xyz), O.morton_encode_batch(xyz))
    assert np.array_equal(D.decode(D.morton(xyz)), xyz)
    assert int(D.morton(np.array([[(1 << 21) - 1] * 3]))[0]) == (1 << 63) - 1


@pytest.mark.parametrize("levels", D.DEPTHS)
def test_deep_scene_covers_the_extreme_codes(O, levels):
    """voxels on coordinate 0 and 2^L - 1 on every axis (Morton bits 3L-3 .. 3L-1 set), a non-trivial emission share"""
    s = D.scene(levels)
    sc = D.oracle_scene(O, s)
    assert len(sc.morton) == len(s.morton) and np.array_equal(sc.morton, s.morton)
    xyz = D.decode(sc.morton)
    assert (xyz.min(0) == 0).all() and (xyz.max(0) == s.res - 1).all()
    top = np.uint64(7) << np.uint64(3 * levels - 3)
    assert ((sc.morton & top) == top).any()
    assert sc.has_emission == 1 and 0.05 < (sc.attrs[:, 4:7] != 0).any(1).mean() < 0.5
    lo, hi = sc.bounds()
    assert (lo == 0).all() and (hi == np.float32(1.0)).all()


@pytest.mark.parametrize("levels", D.DEPTHS)
def test_oracle_walk_against_float64_dda(O, levels):
    s = D.scene(levels)
    sc = D.oracle_scene(O, s)
    ro, rd, kind, _ = s.short_rays(N_RAYS, seed=levels)
    assert len(ro) == N_RAYS
    got = sc.trace(ro, rd, threads=8)
    m_t = root_slab_margin(s, ro, rd)
    hit, cell, t, axis, clear, graze = dda(s, ro, rd, m_t)
    m_max = m_t.max(1)
    m_vox = m_max * np.linalg.norm(rd.astype(np.float64), axis=1) / float(s.dps)  # the largest margin in voxels along the ray
    ghit = got["t"] != MAXF
    gcell = D.decode(sc.morton[np.where(ghit, got["vIndex"], 0)]).astype(np.int64)

    # unambiguous hits: the float64 voxel, its entry axis (nMajor 1: x, 2: y, 0: z) and t within m
    u = hit & clear
    assert ghit[u].all()
    assert np.array_equal(gcell[u], cell[u])
    assert np.array_equal(got["nMajor"][u], np.array([1, 2, 0])[axis[u]])
    assert (np.abs(got["t"][u].astype(np.float64) - t[u]) <= m_t[u, axis[u]]).all()
    # ambiguous hits: within one voxel.  The fp32 walk may miss the voxel where the ray clips its edge or corner within the margin, and
    # (at 20 and 21 levels, where the margins of flat directions are voxels wide) on a few other rays: at most 1 % of them
    a = hit & ~clear
    assert ghit[a & graze].mean() > 0.5 and (~ghit[a & ~graze]).mean() < (0.001 if levels < 20 else 0.01)
    a &= ghit
    cheb = np.abs(gcell[a] - cell[a]).max(1)
    print("levels %d: ambiguous hits %d, farther than one voxel %d, largest %d" % (levels, a.sum(), (cheb > 1).sum(), cheb.max()))
    if levels < 21:
        assert (cheb <= 1).all()
    else:  # at 21 levels flat directions carry margins of several voxels: the fp32 walk can enter the cluster a few voxels off
        assert (cheb <= 1).mean() > 0.99 and cheb.max() <= 8
    # clear misses (no voxel within m of the ray ahead of its origin) must miss
    cand = np.flatnonzero(~hit)
    clear_miss = cand[misses_by_more_than(s, ro[cand], rd[cand], m_vox[cand])]
    assert len(clear_miss) >= (0.02 * N_RAYS if levels < 20 else 5)  # the margins of flat directions widen with depth: fewer clear misses
    assert not ghit[clear_miss].any()

    # the shares: axis-parallel rays keep off the face's edges; for general directions the fp32 walk decides fewer hits exactly with depth
    general = (kind == D.KIND_GENERAL) & hit
    share = u[general].mean()
    measured, floor = UNAMBIGUOUS_GENERAL[levels]
    print("levels %d: m = %.3g voxel (median, axis-parallel rays), unambiguous share (general) %.3f, hits %d, clear misses %d" % (
        levels, np.median(m_vox[kind == D.KIND_AXIS]), share, hit.sum(), len(clear_miss)))
    assert share >= floor
    assert abs(share - measured) < 0.02, "measured share moved: %.3f (recorded %.3f)" % (share, measured)
    axis_rays = (kind == D.KIND_AXIS) & hit
    assert u[axis_rays].mean() > (0.97 if levels < 20 else 0.5), u[axis_rays].mean()
    # the margin along an axis-parallel ray that starts in a unit grid is about 2^(L-23) voxels
    assert 2.0 ** (levels - 24) <= np.median(m_vox[kind == D.KIND_AXIS]) <= 2.0 ** (levels - 22)
