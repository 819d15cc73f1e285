"""Edges of the persistent-wave traversal's refill and of the exit test of its node-visit loop, on all three node-reference flavours
(embedded DAG, plain non-embedded tree, two-level bricks), against the CPU oracle.

Batch sizes: 1, 36 and 37 put a wave on the exhausted path with a handful of live lanes (36 = 64 - the embedded flavour's refill
threshold: the last size at which a wave that still HAD rays to fetch would leave the loop to refill); 65 is two waves, one of them
nearly empty; 4097 and 150 001 are many waves that each take several 64-ray grabs, so that refills straddle grabs.  Every output --
descents included -- equals the oracle's, and every ray has its result written exactly once (the outputs are compared whole: a ray
without a result keeps the zero the buffers start with, a ray stored twice from two lanes would carry the wrong lane's result)."""
import numpy as np
import pytest

from common import bunny_tris, hdr_bytes, position_colors, probe_camera
from fixtures import bunny256, mv, O  # noqa: F401 (fixtures)
from rays import assert_hits_equal, make_pt, random_rays, secondary_like_rays, upload

pytestmark = pytest.mark.gpu

SIZES = (1, 36, 37, 65, 4097, 150_001)
N_MAX = max(SIZES)
NO_HINT = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope="module")
def rays(O, bunny256):
    """one ray set and ONE oracle trace for all flavours and sizes (a batch of n rays = the first n; a ray's result does not depend on the batch)"""
    ro, rd = random_rays(bunny256, N_MAX, 101)
    # random_rays puts its zero-component directions (traced outside the node-visit loop) first: shuffle, so that the small batches are a mix, and make ray 0
    # -- the one-ray batch -- an ordinary ray from outside aimed at the centre of an existing voxel: one live lane in the visit loop of an exhausted stream
    perm = np.random.default_rng(100).permutation(N_MAX)
    ro, rd = ro[perm], rd[perm]
    lo, hi = bunny256.bounds()
    xyz = np.array(O.morton_decode(int(bunny256.morton[len(bunny256.morton) // 2])), np.float32)
    ro[0] = ((lo + hi) / 2 + (hi - lo).max() * np.array([1.3, 0.9, 1.7])).astype(np.float32)
    rd[0] = (np.asarray(bunny256.origin, np.float32) + (xyz + np.float32(0.5)) * np.float32(bunny256.dps) - ro[0]).astype(np.float32)
    sh = (np.arange(N_MAX) % 3 == 1).astype(np.uint8)
    want = bunny256.trace(ro, rd, sh, threads=8, want_descents=True)
    regular = (rd != 0).all(axis=1)
    assert regular[0] and want["t"][0] != O.MAX_FLOAT and want["descents"][0] >= 8
    assert regular[:36].sum() >= 18 and (want["t"][:36] != O.MAX_FLOAT).sum() >= 4
    assert (want["t"] != O.MAX_FLOAT).sum() > 10_000
    for a in (ro, rd, sh, *want.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ro, rd, sh, want


def head(d, n):
    return {k: v[:n] for k, v in d.items() if isinstance(v, np.ndarray)}


def svo_of(mv, O, bunny256, flavour):
    if flavour == "embedded":
        return upload(mv, bunny256)
    if flavour == "plain":
        nodes = O.build_octree(bunny256.morton, 256, dag=False, embed=False)
        return upload(mv, O.Scene(nodes, bunny256.attrs, bunny256.origin, bunny256.dps, 256, embedded=False), embedded=False)
    tris = bunny_tris()
    origin, dps = bunny256.origin, bunny256.dps
    svo = mv.IntersectorOctreeGPU()
    svo.build(tris.reshape(-1, 3), None, None, None, origin, dps, 256, flags=svo.BUILD_NO_DAG | svo.BUILD_NO_EMBEDDED_MASK)
    return svo


@pytest.mark.parametrize("flavour", ["embedded", "plain", "bricks"])
def test_batch_sizes_around_the_refill_threshold_and_across_grabs(mv, O, bunny256, rays, flavour):
    ro, rd, sh, want = rays
    svo = svo_of(mv, O, bunny256, flavour)
    info = svo.info()
    assert info.flavour == {"embedded": 0, "plain": 1, "bricks": 2}[flavour]
    assert info.numberOfVoxels == len(bunny256.morton)
    for n in SIZES:
        got = svo.intersect(ro[:n], rd[:n], sh[:n], want_descents=True)
        assert len(got["t"]) == n
        assert_hits_equal(head(want, n), got)
        assert (got["vIndex"][sh[:n] == 1] == 0).all()


@pytest.fixture(scope="module")
def secondary(O, bunny256, rays):
    """rays that start on the voxels the first N_MAX rays hit, with the hint the path tracer would pass, and their oracle trace"""
    ro0, rd0, sh0, prim = rays
    # (a shadow ray reports no voxel index: only the other hits can say which voxel a secondary ray starts on)
    prim = {"t": np.where(sh0 == 1, np.float32(O.MAX_FLOAT), prim["t"]), "vIndex": prim["vIndex"]}
    parts = [secondary_like_rays(bunny256, ro0, rd0, prim, 102 + 10 * k) for k in range(5)]  # (the same origins, other directions: enough rays for the largest size)
    ro, rd, hint = (np.concatenate([p[i] for p in parts]) for i in range(3))
    assert len(ro) >= N_MAX
    rng = np.random.default_rng(103)
    sh = (rng.random(len(ro)) < 0.4).astype(np.uint8)
    want = bunny256.trace(ro, rd, sh, threads=8, want_descents=True)
    wild = bunny256.morton[rng.integers(0, len(bunny256.morton), len(ro))].astype(np.uint64)
    mixed = np.where(rng.random(len(ro)) < 0.5, hint, NO_HINT)
    return ro, rd, sh, want, {"right": hint, "wrong": wild, "half missing": mixed}


def test_hinted_batches_around_the_refill_threshold_and_across_grabs(mv, O, bunny256, secondary):
    ro, rd, sh, want, hints = secondary
    svo = upload(mv, bunny256)
    for name, hint in hints.items():
        for n in SIZES:
            got = svo.intersect_hinted(ro[:n], rd[:n], hint[:n], sh[:n])
            assert len(got["t"]) == n, (name, n)
            assert_hits_equal(head(want, n), got)


@pytest.mark.parametrize("hints", [True, False])
def test_small_path_traced_frame_and_counters(mv, O, hints):
    """160x90, 3 steps, default batching and pipelining: frame buffer bit-equal to the oracle's render_pt, the four traversal counters equal"""
    tris = bunny_tris()
    cols, emis = position_colors(tris)
    sc = O.build_scene_from_triangles(tris, 256, cols, emis)
    rgba, hw, hh = O.decode_rgbe(hdr_bytes())
    w, h, iters = 160, 90, 3
    cam = probe_camera(sc.origin, sc.dps, 256, focus=9.0, lens_r=0.05)
    pt = make_pt(mv, O, sc, w, h, rgba, hw, hh)
    pt.set_origin_hints(hints)
    for _ in range(iters):
        pt.step(None, cam)
    got = pt.read_framebuffer()[: w * h]
    H = O.HDRI(rgba, hw, hh, rgba, hw, hh, math_mode=1)
    fb = np.zeros((w * h, 4), np.float32)
    tot = dict(rays=0, descents=0, shadowDescents=0, hits=0)
    for it in range(iters):
        fb, _, cnt = sc.render_pt(H, cam, w, h, it, math_mode=1, fb=fb, threads=8)
        for k in tot:
            tot[k] += cnt[k]
    assert np.array_equal(got, fb)
    st = pt.stats()
    for k in tot:
        assert st[k] == tot[k], (k, st[k], tot[k])
