"""The refill section of the stream kernels at its edges (run with -m gpu): the hint replay on shallow octrees (1 to 7 hint levels), origins on voxel faces,
edges and corners and on the root box, stacked ancestors at every level of the replay and at none, batch sizes around the refill threshold, the wave and the
512-ray grab, and one small path-traced frame through the three ray kinds and the result flush.  Every case against the oracle's walk from the root, bit for
bit, descents included."""
import numpy as np
import pytest

from common import bunny_tris, position_colors, probe_camera
from fixtures import bunny256, hdr, mv, O  # noqa: F401 (fixtures)
from rays import assert_hits_equal, make_pt, random_rays, secondary_like_rays, upload

pytestmark = pytest.mark.gpu

MAXF = np.float32(3.402823466e38)
NO_HINT = np.uint64(0xFFFFFFFFFFFFFFFF)
HINT_MAX = 7  # MVRT_HINT_MAX


def hint_levels(res):
    levels = int(np.log2(res))
    return min(levels - 1, HINT_MAX)


def voxel_xyz(morton, levels):
    xyz = np.zeros((len(morton), 3), np.int64)
    for b in range(levels):
        for a in range(3):
            xyz[:, a] |= ((morton >> np.uint64(3 * b + a)) & np.uint64(1)).astype(np.int64) << b
    return xyz


def secondary_set(sc, svo, n_primary, seed):
    """rays that start on the voxels primary rays hit, every tenth with a zero direction component (the irregular path), with the hint of that voxel"""
    ro0, rd0 = random_rays(sc, n_primary, seed)
    prim = svo.intersect(ro0, rd0, want_descents=True)
    ro, rd, hint = secondary_like_rays(sc, ro0, rd0, prim, seed + 1)
    rows = np.arange(0, len(rd), 10)
    rd[rows, (rows // 10) % 3] = 0.0
    sh = (np.random.default_rng(seed + 2).random(len(ro)) < 0.4).astype(np.uint8)
    return ro, rd, hint, sh


def assert_non_trivial(O, want, rd, min_each):
    """hits, misses and irregular rays (a zero direction component) are all present under the oracle alone"""
    hit = want["t"] != O.MAX_FLOAT
    assert hit.sum() >= min_each and (~hit).sum() >= min_each, (int(hit.sum()), int((~hit).sum()))
    assert (rd == 0).any(axis=1).sum() >= min_each


def replay_model(sc, ro, rd, morton):
    """float32 restatement of setupRay and of the walk down the hint's path, only to SORT rays (the expected results are the oracle's): per ray the number of
    levels it follows the hint and the mask of the levels at which a later candidate exists, i.e. at which the replay stacks the ancestor"""
    f32 = np.float32
    lo, hi = sc.bounds()
    levels = int(np.log2(sc.grid_res))
    P = hint_levels(sc.grid_res)
    hint = (morton >> np.uint64(3 * (levels - P))).astype(np.int64)
    with np.errstate(all="ignore"):
        inv = (f32(1.0) / rd).astype(f32)
        neg = inv < 0
        vmask = (neg * np.array([1, 2, 4])).sum(1)
        inv = np.where(neg, -inv, inv)
        o = np.where(neg, (lo + hi - ro).astype(f32), ro)
        clamp = MAXF / np.maximum(np.maximum(np.abs(lo - o), np.abs(hi - o)), f32(1.0))
        inv = np.minimum(inv, clamp).astype(f32)
        t0, t1 = ((lo - o) * inv).astype(f32), ((hi - o) * inv).astype(f32)
        dt = (t1 - t0).astype(f32)
        on = np.isfinite(dt).all(1) & (np.abs(t1).max(1) < f32(1.7e38)) & (np.abs(t0).max(1) < f32(1.7e38)) & ~(t1.min(1) < t0.max(1)) & ~(t1.min(1) < 0)
        k, stacked = np.zeros(len(ro), np.int64), np.zeros(len(ro), np.int64)
        for L in range(P):
            t0L = (t1 - dt * f32(2.0 ** -L)).astype(f32)
            S0 = np.maximum(t0L.max(1), f32(0.0))
            tM = (f32(0.5) * (t0L + t1)).astype(f32)
            bits = tM < S0[:, None]
            on &= ((bits * np.array([1, 2, 4])).sum(1) ^ vmask) == ((hint >> (3 * (P - 1 - L))) & 7)
            fx = ~bits[:, 0] & (tM[:, 0] <= np.minimum(t1[:, 1], t1[:, 2]))
            fy = ~bits[:, 1] & (tM[:, 1] < t1[:, 0]) & (tM[:, 1] <= t1[:, 2])
            fz = ~bits[:, 2] & (tM[:, 2] < np.minimum(t1[:, 0], t1[:, 1]))
            stacked |= (on & (fx | fy | fz)).astype(np.int64) << L
            t1 = np.where(on[:, None], np.where(bits, t1, tM), t1).astype(f32)
            k += on
    return k, stacked


@pytest.fixture(scope="module")
def sec256(mv, O, bunny256):
    """the shared 256^3 set: secondary-like rays with their hints, the oracle's results, the uploaded octree"""
    svo = upload(mv, bunny256)
    ro, rd, hint, sh = secondary_set(bunny256, svo, 60_000, 41)
    want = bunny256.trace(ro, rd, sh, threads=8, want_descents=True)
    assert_non_trivial(O, want, rd, 200)
    return svo, ro, rd, hint, sh, want


@pytest.mark.parametrize("res", [4, 8, 16, 64, 128, 256, 512])
def test_shallow_octrees_replay_every_hint_depth(mv, O, bunny256, res):
    """hintLevelsOf = 1, 2, 3, 5, 6, 7, 7: the hint's alignment and the offsets of the prefix tables at every depth a hint can have"""
    assert hint_levels(res) == {4: 1, 8: 2, 16: 3, 64: 5, 128: 6, 256: 7, 512: 7}[res]
    sc = bunny256 if res == 256 else O.build_scene_from_triangles(bunny_tris(), res)
    svo = upload(mv, sc)
    ro, rd, hint, sh = secondary_set(sc, svo, 30_000, 100 + res)
    want = sc.trace(ro, rd, sh, threads=8, want_descents=True)
    assert_non_trivial(O, want, rd, 20)
    assert_hits_equal(want, svo.intersect_hinted(ro, rd, hint, sh))  # the voxel the ray starts on
    rng = np.random.default_rng(res)
    wild = sc.morton[rng.integers(0, len(sc.morton), len(ro))].astype(np.uint64)
    assert_hits_equal(want, svo.intersect_hinted(ro, rd, wild, sh))  # unrelated voxels that exist
    mixed = np.where(rng.random(len(ro)) < 0.5, hint, NO_HINT)
    assert_hits_equal(want, svo.intersect_hinted(ro, rd, mixed, sh))  # half of the rays without a hint


def test_origins_on_voxel_and_root_box_boundaries(mv, O, bunny256):
    """origins exactly on a voxel's faces, edges and corners and on the faces of the root box, directions with zero and -0 components and along the axes, each
    with the hint of the voxel it was made from; and origins outside the box with a hint (the box-behind-the-origin guard is the root visit's)"""
    sc = bunny256
    svo = upload(mv, sc)
    lo, hi = sc.bounds()
    dps = np.float32(sc.dps)
    rng = np.random.default_rng(5)
    vox = sc.morton[rng.integers(0, len(sc.morton), 400)].astype(np.uint64)
    xyz = voxel_xyz(vox, 8)
    offs = [(a, b, c) for a in (0.0, 0.5, 1.0) for b in (0.0, 0.5, 1.0) for c in (0.0, 0.5, 1.0) if (a, b, c) != (0.5, 0.5, 0.5)]  # 6 faces, 12 edges, 8 corners
    dirs = np.array([(1, 0, 0), (0, -1, 0), (0, 0, 1), (-1, 0, 0), (1, 1, 0), (0, 1, -1), (-0.0, 1, 1), (1, -0.0, -1), (1, 1, -0.0), (-0.0, -0.0, 1),
                     (1, 1, 1), (-1, -1, -1), (1, -2, 0.5), (-0.3, 0.7, 0.2), (0.1, -0.9, -0.4), (-1, 0.25, 2)], np.float32)
    ros, rds, hints = [], [], []
    for i, v in enumerate(xyz):
        for j, o in enumerate(offs):
            ros.append(lo + (v.astype(np.float32) + np.array(o, np.float32)) * dps)
            rds.append(dirs[(i + j) % len(dirs)])
            hints.append(vox[i])
    n_vox = len(ros)
    for i in range(600):  # on the faces of the root box (one coordinate exactly lo or hi), with the hint of some voxel
        p = (lo + rng.random(3).astype(np.float32) * (hi - lo)).astype(np.float32)
        a = i % 3
        p[a] = lo[a] if (i // 3) % 2 else hi[a]
        ros.append(p)
        rds.append(dirs[i % len(dirs)] if i % 2 else (lo + rng.random(3).astype(np.float32) * (hi - lo) - p).astype(np.float32))
        hints.append(vox[i % len(vox)])
    n_box = len(ros)
    for i in range(600):  # outside the box, towards it and away from it, hinted all the same
        p = ((lo + hi) / 2 + (rng.random(3).astype(np.float32) - 0.5) * (hi - lo) * np.float32(3.0)).astype(np.float32)
        tgt = (lo + rng.random(3).astype(np.float32) * (hi - lo)).astype(np.float32)
        d = (tgt - p if i % 3 else p - tgt).astype(np.float32)
        if i % 5 == 0:
            d[i % 3] = 0.0
        ros.append(p)
        rds.append(d)
        hints.append(vox[i % len(vox)])
    ro, rd, hint = np.array(ros, np.float32), np.array(rds, np.float32), np.array(hints, np.uint64)
    assert (np.signbit(rd) & (rd == 0)).any() and ((rd == 0).sum(1) == 2).any()  # -0 components and axis-parallel directions are in the set
    want = sc.trace(ro, rd, None, threads=8, want_descents=True)
    for a, b in ((0, n_vox), (n_vox, n_box), (n_box, len(ro))):  # each group has hits, misses and irregular rays of its own
        assert_non_trivial(O, {"t": want["t"][a:b]}, rd[a:b], 20)
    assert_hits_equal(want, svo.intersect_hinted(ro, rd, hint))
    assert_hits_equal(want, svo.intersect_hinted(ro, rd, np.roll(hint, 7)))  # and with the hint of another voxel


def test_stacked_ancestors_at_every_level_and_at_none(O, bunny256, sec256):
    """the replay stacks an ancestor where a later candidate exists: rays that stack at level 0, 1, ... 6, rays that follow the hint all the way and stack
    nothing, rays that leave the hint's path at once -- sorted on the CPU from the geometry, each set non-empty, each equal to the oracle's walk"""
    svo, ro, rd, hint, sh, want = sec256
    k, stacked = replay_model(bunny256, ro, rd, hint)
    got = svo.intersect_hinted(ro, rd, hint, sh)
    sets = {"level %d" % L: (stacked >> L) & 1 == 1 for L in range(HINT_MAX)}
    sets["all seven levels, nothing stacked"] = (k == HINT_MAX) & (stacked == 0)
    sets["all seven levels stacked"] = stacked == 2 ** HINT_MAX - 1
    sets["off the path at the root"] = (k == 0) & np.isfinite(rd).all(1) & (rd != 0).all(1)
    for name, m in sets.items():
        assert m.sum() > 0, name
        assert_hits_equal({f: want[f][m] for f in ("t", "nMajor", "vIndex", "descents")}, {f: got[f][m] for f in ("t", "nMajor", "vIndex", "descents")})
    assert_hits_equal(want, got)


@pytest.mark.parametrize("n", [1, 27, 28, 29, 63, 64, 65, 511, 512, 513, 1025])
def test_batch_sizes_around_the_threshold_the_wave_and_the_grab(sec256, n):
    svo, ro, rd, hint, sh, want = sec256
    s = slice(1000, 1000 + n)
    assert_hits_equal({f: want[f][s] for f in ("t", "nMajor", "vIndex", "descents")}, svo.intersect_hinted(ro[s], rd[s], hint[s], sh[s]))
    assert_hits_equal({f: want[f][s] for f in ("t", "nMajor", "vIndex", "descents")}, svo.intersect(ro[s], rd[s], sh[s], want_descents=True))


def test_first_wave_of_rays_all_miss_the_root_box(O, bunny256, sec256):
    """every ray of the first load misses the root box: the wave goes round the refill again before its first visit"""
    svo, ro, rd, hint, sh, want = sec256
    lo, hi = bunny256.bounds()
    away = np.tile((hi + (hi - lo)).astype(np.float32), (64, 1))
    away_rd = np.tile(np.array([1.0, 0.5, 0.25], np.float32), (64, 1))
    miss = bunny256.trace(away, away_rd, None, threads=1, want_descents=True)
    assert (miss["t"] == O.MAX_FLOAT).all() and (miss["descents"] == 0).all()
    for tail in (0, 1, 200):
        r0, r1, h = np.concatenate([away, ro[:tail]]), np.concatenate([away_rd, rd[:tail]]), np.concatenate([hint[:64], hint[:tail]])
        s = np.concatenate([np.zeros(64, np.uint8), sh[:tail]])
        w = {f: np.concatenate([miss[f], want[f][:tail]]) for f in ("t", "nMajor", "vIndex", "descents")}
        assert_hits_equal(w, svo.intersect_hinted(r0, r1, h, s))


def test_small_path_traced_frame_one_step_per_pass(mv, O, hdr):
    """64x36, two steps, one step per pass, HDRI and emissive voxels: bounce, shadow and extra rays go through the load and the flush; frame and counters bit for bit"""
    rgba, hw, hh = hdr
    tris = bunny_tris()
    cols, emis = position_colors(tris)
    sc = O.build_scene_from_triangles(tris, 256, cols, emis)
    w, h = 64, 36
    cam = probe_camera(sc.origin, sc.dps, 256, focus=9.0, lens_r=0.05)
    pt = make_pt(mv, O, sc, w, h, rgba, hw, hh)
    pt.set_batch_steps(1)
    H = O.HDRI(rgba, hw, hh, rgba, hw, hh, math_mode=1)
    fb = np.zeros((w * h, 4), np.float32)
    tot = dict(rays=0, shadowRays=0, descents=0, shadowDescents=0, hits=0, samples=0)
    for it in range(2):
        pt.step(None, cam)
        fb, _, cnt = sc.render_pt(H, cam, w, h, it, math_mode=1, fb=fb, threads=8)
        for f in tot:
            tot[f] += cnt[f]
    assert np.array_equal(pt.read_framebuffer()[: w * h], fb)
    st = pt.stats()
    for f in tot:
        assert st[f] == tot[f], (f, st[f], tot[f])
    assert tot["shadowRays"] > 0 and tot["rays"] > tot["samples"] + tot["shadowRays"]  # all three kinds were traced
