"""The survivor scan and the shade kernel's slot numbering without LDS (kernels_rt.hip: kScanTiles / kScanTop, kPtShade with one wave per 256-path block).

Nothing here looks at timing or placement: the offsets must be the integers they always were.  The scan's seams are its tile of T = 256 block counts
(MVRT_SCAN_TILE: one wave, four counts per lane), the C = 256 tile sums one iteration of the top kernel takes (SCAN_TOP_TILES), and the 16-byte quads both load;
a block is 256 flags, so the sizes below are multiples of 256, 256 * T and 256 * T * C, give or take one."""
import numpy as np
import pytest

import adaptive_expected as X
from common import bunny_tris, position_colors, probe_camera
from fixtures import hdr, mv, O  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

BLOCK, T, C = 256, 256, 256
COUNTERS = ("samples", "rays", "shadowRays", "descents", "shadowDescents", "hits")


@pytest.fixture(scope="module")
def scene(O):
    tris = bunny_tris()
    cols, emis = position_colors(tris)
    sc = O.build_scene_from_triangles(tris, 256, cols, emis)
    assert sc.has_emission == 1
    return sc


@pytest.fixture(scope="module")
def Hd(O, hdr):
    rgba, hw, hh = hdr
    return O.HDRI(rgba, hw, hh, rgba, hw, hh, math_mode=1)


def make_pt(mv, sc, w, h, hdr):
    rgba, hw, hh = hdr
    pt = mv.PathTracer()
    pt.setup(None)
    pt.resizeFrameBufferIfNeeded(None, w, h)
    pt.loadHDRIPixels(None, rgba, hw, hh, rgba, hw, hh)
    pt.m_intersectorOctreeGPU.upload(sc.nodes, sc.attrs, sc.origin, sc.dps, sc.grid_res, sc.has_emission)
    return pt


# ---- 1. the scan, through mvrt_compact_indices (host-count form of the same two launches) ---------------------------------------------------------
SIZES = [1, 63, 64, 65, 255, 256, 257,
         BLOCK * T - 1, BLOCK * T, BLOCK * T + 1,  # one tile, give or take a flag: the second tile appears
         BLOCK * 6 + 5,  # 7 blocks: the last quad of counts is partial
         BLOCK * T * 5 + 77,  # 6 tiles: the last quad of tile sums is partial, and so is the last tile's last quad (1281 blocks)
         BLOCK * T * C - 1, BLOCK * T * C, BLOCK * T * C + 1]  # one iteration of the top kernel, give or take a flag: the carry into a second one (16.8 M flags)


def patterns(n):
    rng = np.random.default_rng(n)
    every = np.zeros(n, np.uint8)
    every[::256] = 1
    return [("all", np.ones(n, np.uint8)), ("none", np.zeros(n, np.uint8)), ("every 256th", every), ("random 1 %", (rng.random(n) < 0.01).astype(np.uint8)),
            ("random 99 %", (rng.random(n) < 0.99).astype(np.uint8))]


@pytest.mark.parametrize("n", SIZES)
def test_compact_indices_equal_a_cumulative_sum(mv, n):
    for name, keep in patterns(n):
        incl = np.cumsum(keep, dtype=np.uint64)
        want = np.where(keep != 0, incl - 1, 0xFFFFFFFF).astype(np.uint32)
        dst, kept = mv.compact_indices(keep)
        assert kept == int(incl[-1]), (name, kept, int(incl[-1]))
        bad = np.nonzero(dst != want)[0]
        assert len(bad) == 0, "%s: %d of %d indices differ, first at %s: %s, expected %s" % (name, len(bad), n, bad[:4], dst[bad[:4]], want[bad[:4]])


# ---- 2. the shade kernel's slots at 17 x 13 pixels: 3536 samples per step = 13 blocks + 208, a block that ends in a partial wave -------------------------
def odd_mask(w, h):
    m = np.random.default_rng(1713).random(w * h) < 0.6
    if m.sum() % 2 == 0:
        m[np.nonzero(m)[0][0]] = False
    assert m.sum() % 2 == 1
    return m


@pytest.mark.parametrize("batch,masked", [(1, False), (3, False), (3, True)])
def test_survivor_lists_and_frame_at_17x13(mv, O, scene, hdr, Hd, batch, masked):
    """every stage's survivor list (debug capture) is the oracle's stable filter -- slot j holds the j-th surviving sample in ascending sample order -- and the frame
    buffer is the oracle's bit for bit; under a mask the samples are numbered over the active pixels (an odd number of them), as the library numbers them"""
    w, h = 17, 13
    n = w * h
    mask = odd_mask(w, h) if masked else None
    active = np.arange(n) if mask is None else np.nonzero(mask)[0]
    cams = [probe_camera(scene.origin, scene.dps, 256, focus=9.0, lens_r=0.03, offset=(6 - 0.4 * i, 4, 6)) for i in range(batch)]
    pt = make_pt(mv, scene, w, h, hdr)
    pt.set_batch_steps(batch)
    pt.set_debug_capture(True)
    if masked:
        assert pt.set_sample_mask(mask) == len(active)
    for c in cams:
        pt.step(None, c)
    exp = X.Expected(O, scene, Hd, w, h, aovs=False)
    hits = np.zeros((batch, n * 16), np.uint8)
    for it, c in enumerate(cams):
        exp.step(c, mask)
        scene.render_pt(Hd, c, w, h, it, math_mode=1, threads=8, path_hits=hits[it])
    flat = hits.reshape(batch, n, 16)[:, active].reshape(-1)  # sample id = (step * active pixels + slot) * 16 + spp
    total = 0
    for s in range(8):
        got = pt.debug_stage_survivors(s, batch * len(active) * 16)
        assert np.array_equal(got, np.nonzero(flat > s)[0].astype(np.uint32)), s
        total += len(got)
    assert total > 0 and (flat > 1).any()
    got = pt.read_framebuffer()[:n]
    assert np.array_equal(got.view(np.uint32), exp.fb.view(np.uint32))


# ---- 3. more than one scan tile in the path tracer: 512 x 288 = 9216 blocks per step -----------------------------------------------------------------
def test_frame_of_512x288_equals_the_unpipelined_unbatched_frame(mv, scene, hdr):
    """a 4-step frame as the library schedules it by default (passes of merged steps in flight on its streams; the second frame knows the frame length) against the
    same frame with pipeline depth 1 and batch 1: frame buffer and ray statistics bit for bit"""
    w, h, steps = 512, 288, 4
    cam = probe_camera(scene.origin, scene.dps, 256, focus=9.0, lens_r=0.05)
    out = []
    for serial in (False, True):
        pt = make_pt(mv, scene, w, h, hdr)
        if serial:
            pt.set_pipeline_depth(1)
            pt.set_batch_steps(1)
        for frame in range(2):
            pt.clearFrameBuffer(None)
            for _ in range(steps):
                pt.step(None, cam)
        st = pt.stats()
        out.append((pt.read_framebuffer()[: w * h].copy(), {k: st[k] for k in COUNTERS}))
    assert np.array_equal(out[0][0].view(np.uint32), out[1][0].view(np.uint32))
    assert out[0][1] == out[1][1], (out[0][1], out[1][1])
    assert out[0][0][:, 3].min() == 16 * steps and out[0][1]["rays"] > out[0][1]["samples"]
