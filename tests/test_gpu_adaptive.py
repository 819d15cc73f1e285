"""The sample mask (mvrt_pt_set_sample_mask) and the error mask (mvrt_pt_error_mask) on the GPU against tests/adaptive_expected.py, which builds the expected
buffers from oracle primitives (pinned by tests/test_adaptive_cpu.py).  The setup is that of tests/test_gpu_aov.py: bunny 256^3 with position colours and
emission, the golden HDR, thin lens on.  Every comparison is bit for bit."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import common
import adaptive_expected as X
import denoise_expected as D
from common import GOLDEN, bunny_tris, position_colors, probe_camera
from fixtures import hdr, mv, O  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SIZES = [(128, 72), (100, 37)]  # 36 whole 256-pixel blocks; 15 blocks, the last one 116 pixels and 140 of padding
MASKS = ["random", "checker", "block", "first", "last"]
# the camera of each size: the bunny from afar at 128 x 72, from close by at 100 x 37, where the far view leaves fewer than 20 partly covered pixels under the 1/4 mask
# (checked with the oracle: the statistics test_masked_steps_bit_exact prints and asserts)
OFFSET = {(128, 72): (6, 4, 6), (100, 37): (-2.5, 1.5, -2.0)}


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


def make_pt(mv, sc, w, h, hdr, tile=(0, 1), aovs=True, moments=True):
    rgba, hw, hh = hdr
    pt = mv.PathTracer()
    pt.setup(None)
    pt.set_tile(*tile)
    if aovs:
        pt.set_aovs(True)
    if moments:
        pt.set_moments(True)
    pt.resizeFrameBufferIfNeeded(None, w, h)
    pt.loadHDRIPixels(None, rgba, hw, hh, rgba, hw, hh)
    pt.m_intersectorOctreeGPU.upload(sc.nodes, sc.attrs, sc.origin, sc.dps, sc.grid_res, sc.has_emission)
    return pt


def camera(scene, off=(6, 4, 6)):
    return probe_camera(scene.origin, scene.dps, 256, focus=9.0, lens_r=0.05, offset=off)


def make_mask(kind, w, h):
    """bool per pixel of the frame (global order)"""
    n = w * h
    p = np.arange(n)
    if kind == "random":
        return np.random.default_rng(12345 + w).random(n) < 0.25
    if kind == "checker":
        return ((p % w) + (p // w)) % 2 == 0
    if kind == "block":  # the last 256-pixel block of the frame (whole at 128 x 72, partly padding at 100 x 37)
        return p >= (n - 1) // 256 * 256
    if kind == "first":
        return p == 0
    assert kind == "last"
    return p == n - 1


def read_all(pt):
    """the four accumulation buffers, every owned pixel"""
    return pt.read_framebuffer(), pt.read_aov(pt.AOV_ALBEDO), pt.read_aov(pt.AOV_NORMAL_DEPTH), pt.read_moments()


def assert_same(got, want, what):
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(1))[0]
    assert len(bad) == 0, "%s: %d of %d pixels differ, first %s: %s vs %s" % (what, len(bad), len(got), bad[:4], got[bad[:2]], want[bad[:2]])


def assert_buffers(pt, exp, what=""):
    """frame buffer, feature buffers, moments == expected; the padding of the owned-pixel layout is zero"""
    n = exp.W * exp.H
    for got, want, name in zip(read_all(pt), (exp.fb, exp.albedo, exp.normal_depth, exp.moments), ("frame buffer", "albedo", "normal/depth", "moments")):
        assert got.shape == (pt.owned_pixels(), 4)
        assert_same(got[:n], want, "%s %s" % (what, name))
        assert not got[n:].any(), "%s %s: padding" % (what, name)


# ---- 1. parity ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("w,h", SIZES)
def test_masked_steps_bit_exact(mv, O, scene, hdr, Hd, w, h, kind):
    """one unmasked step, then two under the mask: all four buffers and the per-sample radiance (compact numbering) == expected, inactive pixels keep the bits they
    had, the padding stays zero, w is 16 or 48.  For the random and checkerboard masks the inputs are checked too, so that the test cannot pass empty: 10-90 % of
    the pixels active, >= 5 % of the active samples hit, >= 20 active pixels partly covered, >= 20 active pixels miss entirely."""
    n = w * h
    cam = camera(scene, OFFSET[w, h])
    mask = make_mask(kind, w, h)
    pt = make_pt(mv, scene, w, h, hdr)
    exp = X.Expected(O, scene, Hd, w, h)
    assert pt.active_pixels() == n
    pt.step(None, cam)
    exp.step(cam)
    assert np.array_equal(pt.sample_radiance(n * 16), exp.samples)
    before = read_all(pt)
    assert pt.set_sample_mask(mask) == mask.sum() == pt.active_pixels()
    for it in (1, 2):
        pt.step(None, cam)
        t = exp.step(cam, mask)
        assert np.array_equal(pt.sample_radiance(int(mask.sum()) * 16), exp.samples), it
        if kind in ("random", "checker"):
            share, hits, partly, missing = X.mask_statistics(t, mask)
            print("%s %dx%d iteration %d: %.1f %% active, %.1f %% of the active samples hit, %d partly covered, %d miss entirely" % (kind, w, h, it, 100 * share, 100 * hits, partly,
                                                                                                                                      missing))
            assert 0.10 <= share <= 0.90 and hits >= 0.05 and partly >= 20 and missing >= 20
    assert pt.getSteps() == 3
    assert_buffers(pt, exp, kind)
    after = read_all(pt)
    for a, b in zip(after, before):
        assert np.array_equal(a[:n][~mask].view(np.uint32), b[:n][~mask].view(np.uint32))  # inactive: no bit changed
    assert np.array_equal(after[0][:n, 3], np.where(mask, 48, 16))
    assert pt.stats()["samples"] == (n + 2 * int(mask.sum())) * 16


# ---- 2. all active, none active -------------------------------------------------------------------------------------------------------------------
def test_all_ones_equals_no_mask_and_all_zero_spends_nothing(mv, O, scene, hdr, Hd):
    w, h = SIZES[1]
    n = w * h
    cam = camera(scene, OFFSET[w, h])
    plain, ones = make_pt(mv, scene, w, h, hdr), make_pt(mv, scene, w, h, hdr)
    assert ones.set_sample_mask(np.ones(n, np.uint8)) == n == ones.active_pixels()
    for _ in range(2):
        plain.step(None, cam)
        ones.step(None, cam)
    assert np.array_equal(plain.sample_radiance(n * 16), ones.sample_radiance(n * 16))  # (the first step of the last pass)
    for a, b in zip(read_all(plain), read_all(ones)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    exp = X.Expected(O, scene, Hd, w, h)
    exp.step(cam)
    exp.step(cam)
    assert_buffers(ones, exp, "all ones")
    before = read_all(ones)
    assert ones.set_sample_mask(np.zeros(n, np.uint8)) == 0 and ones.active_pixels() == 0
    spent = ones.stats()["samples"]
    ones.step(None, cam)
    ones.step(None, cam)
    assert ones.getSteps() == 4 and ones.stats()["samples"] == spent
    for a, b in zip(read_all(ones), before):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # the iterations were spent: the next unmasked step is iteration 4
    assert ones.set_sample_mask(None) == n
    ones.step(None, cam)
    exp.steps = 4
    exp.step(cam)
    assert_buffers(ones, exp, "after the empty steps")


# ---- 3. order under batching ----------------------------------------------------------------------------------------------------------------------
def test_masks_keep_step_order_under_batching_and_pipelining(mv, O, scene, hdr, Hd):
    """8 steps with a camera that moves every step -- 2 unmasked, 3 under mask A, 2 under mask B, 1 unmasked -- with the defaults (merged steps, pipelined and sibling
    passes) and with one step per pass on the caller's stream: both == expected"""
    w, h = 64, 40
    n = w * h
    cams = [probe_camera(scene.origin, scene.dps, 256, focus=9.0 + 0.1 * i, lens_r=0.02 * i, offset=(6 - 0.2 * i, 4, 6 + 0.1 * i)) for i in range(8)]
    rng = np.random.default_rng(7)
    A, B = rng.random(n) < 0.3, rng.random(n) < 0.6
    plan = [None, None, A, A, A, B, B, None]
    exp = X.Expected(O, scene, Hd, w, h)
    for c, m in zip(cams, plan):
        exp.step(c, m)
    assert len(np.unique(exp.fb[:, 3])) >= 4 and len(np.unique(exp.albedo[:, 3])) > 8  # mixed sample counts, partial coverage: the order of additions matters
    got = []
    for serial in (False, True):
        pt = make_pt(mv, scene, w, h, hdr)
        if serial:
            pt.set_batch_steps(1)
            pt.set_pipeline_depth(1)
        current = None
        for c, m in zip(cams, plan):
            if m is not current:
                assert pt.set_sample_mask(m) == (n if m is None else m.sum())
                current = m
            pt.step(None, c)
        assert pt.getSteps() == 8
        assert_buffers(pt, exp, "serial" if serial else "default batching")
        got.append(read_all(pt))
    for a, b in zip(*got):
        assert np.array_equal(a, b)


# ---- 4. tiles ---------------------------------------------------------------------------------------------------------------------------------------
def test_masked_tile_shares_assemble_to_the_frame(mv, O, scene, hdr, Hd):
    """2 tile shares at 100 x 37, each under the part of one frame-wide mask that falls on its own pixels: assembled == one handle == expected"""
    from massivevoxelraytracing_amd import tiles
    w, h = SIZES[1]
    n = w * h
    cam = camera(scene, OFFSET[w, h])
    mask = make_mask("random", w, h)
    exp = X.Expected(O, scene, Hd, w, h)
    exp.step(cam)
    exp.step(cam, mask)
    exp.step(cam, mask)
    full = make_pt(mv, scene, w, h, hdr)
    full.step(None, cam)
    full.set_sample_mask(mask)
    full.step(None, cam)
    full.step(None, cam)
    assert_buffers(full, exp, "one tile")
    owned = tiles.owned_pixels(w, h, 2)
    shares, active = [], 0
    for r in range(2):
        pt = make_pt(mv, scene, w, h, hdr, tile=(r, 2))
        assert pt.owned_pixels() == owned
        g = tiles.global_pixel_index(w, h, r, 2)
        local = np.zeros(owned, np.uint8)
        local[g >= 0] = mask[g[g >= 0]]
        pt.step(None, cam)
        active += pt.set_sample_mask(local)
        pt.step(None, cam)
        pt.step(None, cam)
        shares.append(pt)
    assert active == mask.sum()
    d_g = mv.DeviceArray((2, owned, 4), f32)
    for r, pt in enumerate(shares):
        pt.join(None)
        mv.memcpy_d2d(d_g.ptr + r * owned * 16, pt.framebuffer_dev(), owned * 16)
    d_f = mv.DeviceArray((n, 4), f32)
    mv.assemble_tiles(d_g, 2, owned, w, h, d_f)
    mv.synchronize()
    assert_same(d_f.to_host(), exp.fb, "assembled frame buffer")
    assert np.array_equal(d_f.to_host(), full.read_framebuffer()[:n])
    for want, read in ((exp.albedo, lambda p: p.read_aov(p.AOV_ALBEDO)), (exp.normal_depth, lambda p: p.read_aov(p.AOV_NORMAL_DEPTH)), (exp.moments, lambda p: p.read_moments())):
        assert_same(tiles.assemble(np.stack([read(p) for p in shares]), w, h), want, "assembled")


# ---- 5. lifetime --------------------------------------------------------------------------------------------------------------------------------------
def test_mask_lifetime(mv, O, scene, hdr, Hd):
    """dropped by clearFrameBuffer (the next step samples every pixel), by a reallocating resize and by set_tile; kept across updateScene; active_pixels follows"""
    w, h = 64, 40
    n = w * h
    cam = camera(scene)
    mask = make_mask("checker", w, h)
    pt = make_pt(mv, scene, w, h, hdr)
    assert pt.set_sample_mask(mask) == n // 2 == pt.active_pixels()
    pt.step(None, cam)
    assert (pt.read_framebuffer()[:n, 3] == np.where(mask, 16, 0)).all()
    pt.clearFrameBuffer(None)
    assert pt.active_pixels() == n
    pt.step(None, cam)
    exp = X.Expected(O, scene, Hd, w, h)
    exp.step(cam)
    assert_buffers(pt, exp, "after clear")
    # kept across updateScene (the same triangles: the same octree)
    assert pt.set_sample_mask(mask) == n // 2
    tris = bunny_tris()
    cols, emis = position_colors(tris)
    pt.updateScene(tris.reshape(-1, 3), cols.reshape(-1, 3), emis.reshape(-1, 3), None, scene.origin, scene.dps, 256)
    assert pt.active_pixels() == n // 2
    pt.step(None, cam)
    exp.step(cam, mask)
    assert_buffers(pt, exp, "after updateScene")
    # a resize to the same size keeps it, one that reallocates drops it
    pt.resizeFrameBufferIfNeeded(None, w, h)
    assert pt.active_pixels() == n // 2
    pt.resizeFrameBufferIfNeeded(None, 48, 30)
    assert pt.active_pixels() == 48 * 30 and pt.getSteps() == 0
    pt.step(None, cam)
    assert (pt.read_framebuffer()[: 48 * 30, 3] == 16).all()
    # set_tile leaves no frame and no mask
    assert pt.set_sample_mask(np.ones(48 * 30, np.uint8)) == 48 * 30
    pt.set_tile(0, 2)
    assert pt.active_pixels() == 0
    with pytest.raises(mv.MvrtError, match="no frame buffer"):
        pt.set_sample_mask(None)
    pt.resizeFrameBufferIfNeeded(None, 48, 30)
    assert pt.active_pixels() == 768  # 6 blocks of 1440 pixels: this rank owns blocks 0, 2, 4, all whole
    pt.step(None, cam)
    assert (pt.read_framebuffer()[:768, 3] == 16).all()


# ---- 6. error mask --------------------------------------------------------------------------------------------------------------------------------------
def test_error_mask_matches_the_formula(mv, O, scene, hdr):
    """after 2 and after 4 unmasked steps: bytes and count == the formula on the buffers read back, strictly between none and all; min_samples above the count marks
    every valid pixel, max_samples at the count none; the padding is 0; the call sets no mask"""
    w, h = SIZES[1]
    n = w * h
    cam = camera(scene, OFFSET[w, h])
    pt = make_pt(mv, scene, w, h, hdr, aovs=False)
    threshold = 0.1
    for steps in (2, 4):
        pt.step(None, cam)
        pt.step(None, cam)
        got, count = pt.error_mask(threshold, min_samples=16)
        fb, mo = pt.read_framebuffer(), pt.read_moments()
        want = X.error_mask(fb[:n], mo[:n], threshold, 0.01, 16, 0)
        print("%d steps: %d of %d pixels above %.2f" % (steps, count, n, threshold))
        assert got.shape == (pt.owned_pixels(),) and got.dtype == np.uint8
        assert np.array_equal(got[:n], want) and not got[n:].any() and count == want.sum()
        assert 0 < count < n
        spp = 16 * steps
        got, count = pt.error_mask(threshold, min_samples=spp + 1)
        assert (got[:n] == 1).all() and not got[n:].any() and count == n
        got, count = pt.error_mask(threshold, min_samples=16, max_samples=spp)
        assert not got.any() and count == 0
        got, count = pt.error_mask(threshold, lum_floor=0.5, min_samples=16)  # (a floor above most means: fewer pixels pass)
        assert np.array_equal(got[:n], X.error_mask(fb[:n], mo[:n], threshold, 0.5, 16, 0)) and count == got.sum() and 0 < count < want.sum()
        assert pt.active_pixels() == n and pt.getSteps() == steps
    # a device array in, nothing copied back; it feeds set_sample_mask as it is
    d = mv.DeviceArray(pt.owned_pixels(), np.uint8)
    out, count = pt.error_mask(threshold, min_samples=16, out_dev=d)
    assert out is d and np.array_equal(d.to_host()[:n], want)
    assert pt.set_sample_mask(d) == count == pt.active_pixels()
    pt.step(None, cam)
    assert np.array_equal(pt.read_framebuffer()[:n, 3], np.where(want, 80, 64))
    with pytest.raises(mv.MvrtError, match="threshold"):
        pt.error_mask(0.0)


# ---- 7. denoise -----------------------------------------------------------------------------------------------------------------------------------------
def test_denoise_after_masked_steps(mv, O, scene, hdr):
    """per-pixel sample counts: denoise() == the contract applied to the buffers read back"""
    w, h = 64, 40
    n = w * h
    cam = camera(scene)
    pt = make_pt(mv, scene, w, h, hdr)
    pt.step(None, cam)
    pt.step(None, cam)
    mask, count = pt.error_mask(0.1)
    assert 0 < count < n
    pt.set_sample_mask(mask)
    pt.step(None, cam)
    pt.step(None, cam)
    fb, al, nd, mo = (b[:n] for b in read_all(pt))
    assert set(np.unique(fb[:, 3])) == {32, 64}
    pt.denoise(None, iterations=3)
    assert_same(pt.read_denoised(), D.denoise(O, fb, al, nd, mo, w, h, iterations=3), "denoised")


# ---- 8. C++ mirror ----------------------------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_adaptive_members(tmp_path):
    """tests/cpp/adaptive_usage.cpp on the header-only mirror: errorMask, setSampleMask, activePixels"""
    import massivevoxelraytracing_amd as mv
    exe, libdir = common.compile_usage(tmp_path, "adaptive_usage", missing="fail")
    shutil.copy(os.path.join(GOLDEN, "monks_forest_s.hdr"), tmp_path / "monks_forest_s.hdr")
    out = subprocess.check_output([str(exe), "run"], cwd=tmp_path, timeout=300).decode()
    print(out)
    assert "active 2304 of 2304 owned" in out
    line = [l for l in out.split("\n") if l.startswith("marked")][0].split()
    assert line[1] == "2304" and line[2] == "0" and line[3] == line[5] == line[7]
    assert "counts 1 steps 3" in out and "off 2304" in out and "cleared 2304" in out
