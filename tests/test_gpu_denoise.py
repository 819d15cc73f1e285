"""Luminance moments (mvrt_pt_set_moments) and the a-trous denoiser (mvrt_pt_denoise, mvrt_denoise_buffers) on the GPU against tests/denoise_expected.py, which
restates the contract of include/mvrt.h from oracle primitives (its recipe is pinned by tests/test_denoise_cpu.py).  Every comparison is bit for bit."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import common
import aov_expected as A
import denoise_expected as D
from common import GOLDEN, bunny_tris, position_colors, probe_camera
from fixtures import hdr, mv, O  # noqa: F401 (fixtures)
from voxel_mesh_app import write_reader_obj

pytestmark = pytest.mark.gpu

OFFSETS = [(6, 4, 6), (-6, -4, -6), (-2.5, 1.5, -2.0)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def scene(O):
    tris = bunny_tris()
    cols, emis = position_colors(tris)
    return O.build_scene_from_triangles(tris, 256, cols, emis)


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


def camera(scene, off=OFFSETS[0]):
    return probe_camera(scene.origin, scene.dps, 256, focus=9.0, lens_r=0.05, offset=off)


def buffers(pt, n):
    """host copies of the four inputs of the filter"""
    return pt.read_framebuffer()[:n], pt.read_aov(pt.AOV_ALBEDO)[:n], pt.read_aov(pt.AOV_NORMAL_DEPTH)[:n], pt.read_moments()[:n]


assert_same = D.assert_same


# ---- 5. moments -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,iters", [(128, 72, 2), (100, 37, 1)])
def test_moments_bit_exact_and_nothing_else_moves(mv, O, scene, hdr, w, h, iters):
    """moments == the sequential float32 sums over the oracle's per-sample radiance, three cameras; in the same runs the frame buffer, the per-sample radiance
    and both feature buffers are what a handle with the moments off gives; the padding of the owned-pixel layout stays zero"""
    rgba, hw, hh = hdr
    Hd = O.HDRI(rgba, hw, hh, rgba, hw, hh, math_mode=1)
    n = w * h
    for off in OFFSETS:
        cam = camera(scene, off)
        on, plain = make_pt(mv, scene, w, h, hdr), make_pt(mv, scene, w, h, hdr, moments=False)
        assert plain.moments_dev() is None and on.moments_dev()
        exp = D.ExpectedMoments(w, h)
        fb = np.zeros((n, 4), f32)
        for it in range(iters):
            on.step(None, cam)
            plain.step(None, cam)
            fb, sl, _ = scene.render_pt(Hd, cam, w, h, it, math_mode=1, fb=fb, want_samples=True, threads=8)
            exp.step(sl)
            assert np.array_equal(on.sample_radiance()[: n * 16], sl) and np.array_equal(plain.sample_radiance()[: n * 16], sl), (off, it)
        got = on.read_moments()
        assert got.shape == (on.owned_pixels(), 4) and not got[n:].any()
        assert_same(got[:n], exp.moments, "moments, camera %s" % (off,))
        assert (got[:n, 0] > 0).sum() > n // 2 and not got[:, 2:4].any()
        assert np.array_equal(on.read_framebuffer()[:n], fb) and np.array_equal(plain.read_framebuffer(), on.read_framebuffer())
        for which in (on.AOV_ALBEDO, on.AOV_NORMAL_DEPTH):
            assert np.array_equal(on.read_aov(which), plain.read_aov(which))
        # independent of the feature buffers
        alone = make_pt(mv, scene, w, h, hdr, aovs=False)
        for it in range(iters):
            alone.step(None, cam)
        assert_same(alone.read_moments()[:n], exp.moments, "moments without feature buffers")
        assert alone.aov_dev(alone.AOV_ALBEDO) is None


def test_moments_keep_step_order_under_batching_and_pipelining(mv, O, scene, hdr):
    """8 steps with a camera that moves every step: the defaults (merged steps, pipelined and sibling passes) == one step per pass on the caller's stream == expected"""
    rgba, hw, hh = hdr
    Hd = O.HDRI(rgba, hw, hh, rgba, hw, hh, math_mode=1)
    w, h, iters = 64, 40, 8
    cams = [probe_camera(scene.origin, scene.dps, 256, focus=9.0 + 0.1 * i, lens_r=0.02 * i, offset=(6 - 0.2 * i, 4, 6 + 0.1 * i)) for i in range(iters)]
    exp = D.ExpectedMoments(w, h)
    for i, c in enumerate(cams):
        exp.step(scene.render_pt(Hd, c, w, h, i, math_mode=1, want_samples=True, threads=8)[1])
    got = []
    for serial in (False, True):
        pt = make_pt(mv, scene, w, h, hdr)
        if serial:
            pt.set_batch_steps(1)
            pt.set_pipeline_depth(1)
        for c in cams:
            pt.step(None, c)
        assert pt.getSteps() == iters
        got.append(pt.read_moments())
        assert_same(got[-1][: w * h], exp.moments, "serial" if serial else "default batching")
    assert np.array_equal(got[0], got[1])
    # clear zeroes them; set_moments is refused while steps are accumulated
    with pytest.raises(mv.MvrtError, match="clear"):
        pt.set_moments(False)
    pt.clearFrameBuffer(None)
    assert not pt.read_moments().any()
    pt.set_moments(False)
    assert pt.moments_dev() is None
    with pytest.raises(mv.MvrtError, match="mvrt_pt_set_moments"):
        pt.read_moments()


@pytest.mark.parametrize("shares", [2, 3])
def test_moments_of_tile_shares_assemble_to_the_frame(mv, scene, hdr, shares):
    from massivevoxelraytracing_amd import tiles
    w, h = 200, 113
    cam = camera(scene)
    full = make_pt(mv, scene, w, h, hdr)
    full.step(None, cam)
    full.step(None, cam)
    want = full.read_moments()[: w * h]
    assert (want[:, 0] > 0).sum() > w * h // 2
    owned = tiles.owned_pixels(w, h, shares)
    d_g = mv.DeviceArray((shares, owned, 4), np.float32)
    host = []
    for r in range(shares):
        pt = make_pt(mv, scene, w, h, hdr, tile=(r, shares))
        assert pt.owned_pixels() == owned
        pt.step(None, cam)
        pt.step(None, cam)
        pt.join(None)
        mv.memcpy_d2d(d_g.ptr + r * owned * 16, pt.moments_dev(), owned * 16)
        mv.synchronize()
        host.append(pt.read_moments())
    d_f = mv.DeviceArray((w * h, 4), np.float32)
    mv.assemble_tiles(d_g, shares, owned, w, h, d_f)
    mv.synchronize()
    assert_same(d_f.to_host(), want, "%d shares" % shares)
    assert np.array_equal(tiles.assemble(np.stack(host), w, h), want)


# ---- 6. denoiser parity -----------------------------------------------------------------------------------------------------------------------------
PARAM_SETS = [dict(iterations=1), dict(iterations=3), dict(), dict(iterations=8), dict(sigmaNormal=0.3, sigmaDepth=0.2, sigmaCoverage=0.6, sigmaLuminance=0.7, albedoFloor=0.2),
              dict(flags=D.NO_DEMODULATION), dict(iterations=2, flags=D.NO_DEMODULATION, sigmaLuminance=4.0)]


@pytest.mark.parametrize("w,h,iters", [(128, 72, 2), (100, 37, 1)])
def test_denoiser_equals_the_contract(mv, O, scene, hdr, w, h, iters):
    """mvrt_pt_denoise == the numpy restatement of the contract on the buffers of the same handle: both frame sizes, three cameras, 1 / 3 / 5 / 8 iterations, default
    and other sigmas, NO_DEMODULATION.  The inputs are checked, so that the test cannot pass empty."""
    n = w * h
    for off in OFFSETS:
        cam = camera(scene, off)
        pt = make_pt(mv, scene, w, h, hdr)
        for _ in range(iters):
            pt.step(None, cam)
        c, a, nd, m = buffers(pt, n)
        pr = D.prepare(c, a, nd, m, 0.01, 0)
        share = float(a[:, 3].astype(np.float64).sum() / c[:, 3].astype(np.float64).sum())
        partly = int(((a[:, 3] > 0) & (a[:, 3] < c[:, 3])).sum())
        with_var = int((pr["v"][pr["valid"]] > 0).sum())
        print("camera %s %dx%d: %.1f %% of the samples hit, %d partly covered pixels, %d pixels with v > 0" % (off, w, h, 100 * share, partly, with_var))
        assert share >= 0.05 and partly >= 50 and with_var >= 100
        for params in PARAM_SETS:
            pt.denoise(None, **params)
            got = pt.read_denoised()
            want = D.denoise(O, c, a, nd, m, w, h, **params)
            assert_same(got, want, "camera %s, %s" % (off, params))
            if not params:
                hit = pr["valid"]
                noisy = (c[:, 0:3] / c[:, 3:4]).astype(f32)
                changed = (got[hit, 0:3] != noisy[hit]).any(1).sum()
                assert changed >= hit.sum() / 2, (changed, hit.sum())
                assert np.array_equal(got[pr["sky"], 0:3], noisy[pr["sky"]]) and (got[:, 3] == 1).all()


# ---- 7. / 8. the buffers entry point and resolve ----------------------------------------------------------------------------------------------------
def test_denoise_buffers_on_assembled_tiles_and_resolve(mv, O, scene, hdr):
    """four buffers of 3 tile shares, gathered and assembled on the device, through mvrt_denoise_buffers == mvrt_pt_denoise on one handle == the contract;
    mvrt_resolve_buffer of the denoised buffer == the oracle's resolve of the expected one"""
    from massivevoxelraytracing_amd import tiles
    w, h, shares = 128, 72, 3
    n = w * h
    cam = camera(scene)
    full = make_pt(mv, scene, w, h, hdr)
    full.step(None, cam)
    full.step(None, cam)
    full.denoise(None)
    want = full.read_denoised()
    assert_same(want, D.denoise(O, *buffers(full, n), w, h), "one handle")
    owned = tiles.owned_pixels(w, h, shares)
    pts = []
    for r in range(shares):
        pt = make_pt(mv, scene, w, h, hdr, tile=(r, shares))
        pt.step(None, cam)
        pt.step(None, cam)
        pt.join(None)
        with pytest.raises(mv.MvrtError, match="mvrt_denoise_buffers"):
            pt.denoise(None)
        pts.append(pt)
    frames = []
    for get in (lambda p: p.framebuffer_dev(), lambda p: p.aov_dev(p.AOV_ALBEDO), lambda p: p.aov_dev(p.AOV_NORMAL_DEPTH), lambda p: p.moments_dev()):
        d_g = mv.DeviceArray((shares, owned, 4), np.float32)
        for r, pt in enumerate(pts):
            mv.memcpy_d2d(d_g.ptr + r * owned * 16, get(pt), owned * 16)
        d_f = mv.DeviceArray((n, 4), np.float32)
        mv.assemble_tiles(d_g, shares, owned, w, h, d_f)
        mv.synchronize()
        frames.append(d_f)
    before = [f.to_host() for f in frames]
    d_out = mv.DeviceArray((n, 4), np.float32)
    mv.denoise_buffers(*frames, w, h, d_out)
    mv.synchronize()
    assert_same(d_out.to_host(), want, "assembled shares")
    for f, b in zip(frames, before):
        assert np.array_equal(f.to_host(), b)  # the inputs are not modified
    # caller-owned scratch of exactly the stated size, and other parameters
    scratch = mv.DeviceArray(mv.denoise_scratch_bytes(w, h), np.uint8)
    mv.denoise_buffers(*frames, w, h, d_out, scratch, scratch.nbytes, iterations=2, sigmaLuminance=1.0)
    mv.synchronize()
    full.denoise(None, iterations=2, sigmaLuminance=1.0)
    assert_same(d_out.to_host(), full.read_denoised(), "caller's scratch")
    with pytest.raises(mv.MvrtError, match="scratch too small"):
        mv.denoise_buffers(*frames, w, h, d_out, scratch, scratch.nbytes - 1)
    # resolve
    full.denoise(None)
    d_u8 = mv.DeviceArray((n, 4), np.uint8)
    mv.resolve_buffer(full.denoised_dev(), n, d_u8)
    mv.synchronize()
    got = d_u8.to_host()
    assert np.array_equal(got, O.resolve(want, math_mode=1))
    assert len(np.unique(got[:, 0:3])) > 50


# ---- 9. non-interference ----------------------------------------------------------------------------------------------------------------------------
def test_denoise_leaves_the_accumulation_alone(mv, scene, hdr):
    w, h = 100, 37
    n = w * h
    cam = camera(scene)
    a, b = make_pt(mv, scene, w, h, hdr), make_pt(mv, scene, w, h, hdr)
    assert a.denoised_dev() is None
    for pt in (a, b):
        pt.step(None, cam)
        pt.step(None, cam)
    before = buffers(a, a.owned_pixels())
    a.denoise(None)
    first = a.read_denoised()
    assert a.denoised_dev() and a.getSteps() == 2
    for x, y in zip(before, buffers(a, a.owned_pixels())):
        assert np.array_equal(x, y)
    a.step(None, cam)  # pending when the next denoise comes: it is launched first
    a.denoise(None, iterations=3)
    a.step(None, cam)
    for pt in (b, b):
        pt.step(None, cam)
    assert a.getSteps() == b.getSteps() == 4
    for x, y in zip(buffers(a, a.owned_pixels()), buffers(b, b.owned_pixels())):
        assert np.array_equal(x, y)
    b.denoise(None)
    a.denoise(None)
    assert np.array_equal(a.read_denoised(), b.read_denoised()) and not np.array_equal(a.read_denoised(), first)
    # a resize releases the denoised image; the same size does not
    a.resizeFrameBufferIfNeeded(None, w, h)
    assert a.denoised_dev()
    a.resizeFrameBufferIfNeeded(None, 64, 40)
    assert a.denoised_dev() is None
    with pytest.raises(mv.MvrtError, match="no steps"):
        a.denoise(None)
    with pytest.raises(mv.MvrtError, match="mvrt_pt_denoise first"):
        a.read_denoised()
    for flag, word in (("aovs", "mvrt_pt_set_aovs"), ("moments", "mvrt_pt_set_moments")):
        pt = make_pt(mv, scene, 64, 40, hdr, **{flag: False})
        pt.step(None, cam)
        with pytest.raises(mv.MvrtError, match=word):
            pt.denoise(None)
        assert pt.getSteps() == 1


# ---- 10. failure paths ------------------------------------------------------------------------------------------------------------------------------
def test_a_failed_allocation_of_denoise_leaves_the_frame_and_no_denoised_buffer(mv, O, scene, hdr):
    w, h = 100, 37
    n = w * h
    cam = camera(scene)
    pt = make_pt(mv, scene, w, h, hdr)
    pt.step(None, cam)
    pt.step(None, cam)
    mv.synchronize()
    before = buffers(pt, pt.owned_pixels())
    want = D.denoise(O, *[x[:n] for x in before], w, h)
    # how many allocations a first denoise makes: count them on a twin
    twin = make_pt(mv, scene, w, h, hdr)
    twin.step(None, cam)
    twin.join(None)
    mv.synchronize()
    a0 = mv.allocation_state()[2]
    twin.denoise(None)
    made = mv.allocation_state()[2] - a0
    assert made >= 2
    twin.denoise(None)
    assert mv.allocation_state()[2] - a0 == made  # the buffers are kept between calls
    del twin
    live0 = mv.allocation_state()[:2]
    for nth in range(1, made + 1):
        mv.set_test_fail_allocation(nth)
        with pytest.raises(mv.MvrtError, match="mvrt_test_fail_allocation"):
            pt.denoise(None)
        mv.set_test_fail_allocation(0)
        assert pt.denoised_dev() is None and pt.getSteps() == 2
        assert mv.allocation_state()[:2] == live0, nth  # nothing leaked, nothing of the frame released
        for x, y in zip(before, buffers(pt, pt.owned_pixels())):
            assert np.array_equal(x, y)
    pt.denoise(None)
    assert_same(pt.read_denoised(), want, "after the failures")
    # ... and after a successful denoise: a resize releases the image, the reallocation the next denoise needs fails at each of its allocations in turn
    w2, h2 = 64, 40
    assert pt.denoised_dev()
    pt.resizeFrameBufferIfNeeded(None, w2, h2)
    assert pt.denoised_dev() is None
    pt.step(None, cam)
    mv.synchronize()
    before = buffers(pt, pt.owned_pixels())
    live1 = mv.allocation_state()[:2]
    for nth in range(1, made + 1):
        mv.set_test_fail_allocation(nth)
        with pytest.raises(mv.MvrtError, match="mvrt_test_fail_allocation"):
            pt.denoise(None)
        mv.set_test_fail_allocation(0)
        assert pt.denoised_dev() is None and pt.getSteps() == 1 and mv.allocation_state()[:2] == live1, nth
        with pytest.raises(mv.MvrtError, match="mvrt_pt_denoise first"):
            pt.read_denoised()
    for x, y in zip(before, buffers(pt, pt.owned_pixels())):
        assert np.array_equal(x, y)
    pt.denoise(None)
    assert_same(pt.read_denoised(), D.denoise(O, *[x[: w2 * h2] for x in before], w2, h2), "after a resize and the failures")
    assert mv.allocation_state()[0] == live1[0] + made


# ---- 11. C++ mirror and the batch driver ------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_denoise_members(tmp_path):
    """tests/cpp/denoise_usage.cpp on the header-only mirror: setMoments, denoise, m_momentsF32 / m_denoisedF32 re-pointed by everything that reallocates"""
    import massivevoxelraytracing_amd as mv
    exe, libdir = common.compile_usage(tmp_path, "denoise_usage", missing="fail")
    shutil.copy(os.path.join(GOLDEN, "monks_forest_s.hdr"), tmp_path / "monks_forest_s.hdr")
    out = subprocess.check_output([str(exe), "run"], cwd=tmp_path, timeout=300).decode()
    print(out)
    assert "views 1 0 bytes %d" % (64 * 36 * 16) in out
    assert "denoised 1 bytes %d w 1 same 1 steps 2" % (64 * 36 * 16) in out
    assert "refused 1 view 1" in out and "resized 1" in out and "off 1" in out and "tile 1 1" in out


def test_batch_driver_writes_the_denoised_frame(tmp_path, O):
    """rtcamp_batch --denoise: <frame>_denoised == the oracle's resolve of the contract applied to the expected buffers of that frame (the frame is replayed through
    the Python binding from the dumped camera); the frame itself is unchanged by the option"""
    import massivevoxelraytracing_amd as mv
    from massivevoxelraytracing_amd import build as b
    exe = b.build_apps(verbose=False)
    tris = bunny_tris()
    obj = tmp_path / "bunny.obj"
    write_reader_obj(obj, tris)
    hdr_file = os.path.join(GOLDEN, "monks_forest_s.hdr")
    W, H, steps = 96, 54, 2
    outs = {}
    for name, extra in (("plain", []), ("dn", ["--denoise"])):
        out = tmp_path / name
        os.mkdir(out)
        subprocess.check_call([exe, str(obj), hdr_file, str(out), "--frames", "8", "--frame-range", "5", "6", "--size", str(W), str(H), "--res", "64", "256", "--steps", str(steps),
                               "--dump-cameras"] + extra)
        outs[name] = out
    assert open(outs["plain"] / "005.ppm", "rb").read() == open(outs["dn"] / "005.ppm", "rb").read()
    assert not os.path.exists(outs["plain"] / "005_denoised.ppm") and not os.path.exists(outs["dn"] / "005_albedo.ppm")
    lines = open(outs["dn"] / "005.camera.txt").read().split("\n")
    view = np.array([float.fromhex(t) for t in lines[0].split()], np.float32)
    proj = np.array([float.fromhex(t) for t in lines[1].split()], np.float32)
    t = lines[2].split()
    focus, lens_r, ox, oy, oz, dps = (float.fromhex(x) for x in t[:6])
    res = int(t[6])
    # the driver's scene (white mesh, emission on the top of the box) rebuilt by the library itself from the same .obj data
    v = tris.reshape(-1, 3)
    pt = mv.PathTracer()
    pt.setup(None)
    pt.set_aovs(True)
    pt.set_moments(True)
    pt.resizeFrameBufferIfNeeded(None, W, H)
    pt.loadHDRI(None, hdr_file, hdr_file)
    lo = v.min(0)
    wide = float((v.max(0) - lo).max())
    emis = np.zeros_like(v)
    emis[v[:, 1] > lo[1] + np.float32(0.94) * np.float32(wide)] = [1.0, 0.85, 0.6]
    pt.updateScene(v, np.ones_like(v), emis, None, np.array([ox, oy, oz], np.float32), np.float32(dps), res)
    for _ in range(steps):
        pt.step(None, (view, proj), focus, lens_r)
    ppm = open(outs["dn"] / "005.ppm", "rb").read()
    head = len(b"P6\n%d %d\n255\n" % (W, H))
    frame = np.frombuffer(ppm[head:], np.uint8).reshape(H * W, 3)
    assert np.array_equal(frame, pt.toImageAsync()[: W * H, 0:3]), "the replay renders the driver's frame"
    want = O.resolve(D.denoise(O, *buffers(pt, W * H), W, H), math_mode=1)[:, 0:3]
    got = np.frombuffer(open(outs["dn"] / "005_denoised.ppm", "rb").read()[head:], np.uint8).reshape(H * W, 3)
    assert np.array_equal(got, want)
    assert len(np.unique(got)) > 20 and (got != frame).any(1).sum() > 100


# ---- 12. quality at a user's size -------------------------------------------------------------------------------------------------------------------
def test_quality_on_the_dragon_standin(mv):
    """dragon stand-in 1024^3, 512 x 288, inputs of 16 and 64 spp, truth 1024 spp, all rendered here: relMSE( denoised ) < relMSE( noisy ).  The ratios are printed
    and, when MVRT_DENOISE_QUALITY_OUT names a file, written there (profiles/denoise_quality.json comes from such a run)."""
    from massivevoxelraytracing_amd import scenes
    w, h, res = 512, 288, 1024
    n = w * h
    verts, cols, emis = scenes.SCENES["dragon"](1.0)
    origin, dps = scenes.bounding_grid(verts, res)
    pt = mv.PathTracer()
    pt.setup(None)
    pt.set_aovs(True)
    pt.set_moments(True)
    pt.resizeFrameBufferIfNeeded(None, w, h)
    hdr_file = os.path.join(GOLDEN, "monks_forest_s.hdr")
    pt.loadHDRI(None, hdr_file, hdr_file)
    pt.updateScene(verts, cols, emis, None, origin, dps, res)
    info = pt.m_intersectorOctreeGPU.info()
    centre = (np.array(info.lower[:]) + np.array(info.upper[:])) / 2
    eye = centre + np.array([2.6, 1.5, 3.1])
    cam = scenes.look_at_camera(eye, centre, 40.0, float(np.linalg.norm(eye - centre)), 0.02)
    frames = {}
    for it in range(64):
        pt.step(None, cam)
        if it + 1 in (1, 4):
            pt.denoise(None)
            fb = pt.read_framebuffer()[:n]
            frames[16 * (it + 1)] = ((fb[:, 0:3] / fb[:, 3:4]).astype(f32), pt.read_denoised(), pt.read_aov(pt.AOV_ALBEDO)[:n, 3] > 0)
    fb = pt.read_framebuffer()[:n]
    assert (fb[:, 3] == 1024).all()
    truth = (fb[:, 0:3] / fb[:, 3:4]).astype(f32)
    report = {"scene": "dragon stand-in %d^3, %dx%d, truth 1024 spp, default parameters" % (res, w, h), "device": mv.device_name(), "cases": []}
    for spp, (noisy, den, hit) in sorted(frames.items()):
        assert hit.mean() > 0.05
        rn, rd = D.rel_mse(noisy, truth), D.rel_mse(den, truth)
        rnh, rdh = D.rel_mse(noisy, truth, hit), D.rel_mse(den, truth, hit)
        print("%d spp: relMSE noisy %.6f denoised %.6f ratio %.3f; over h > 0: %.6f -> %.6f ratio %.3f" % (spp, rn, rd, rd / rn, rnh, rdh, rdh / rnh))
        report["cases"].append({"spp": spp, "relMSE_noisy": rn, "relMSE_denoised": rd, "ratio": rd / rn, "relMSE_noisy_hit_pixels": rnh, "relMSE_denoised_hit_pixels": rdh,
                                "ratio_hit_pixels": rdh / rnh, "hit_pixel_share": float(hit.mean())})
        assert rd < rn, (spp, rd, rn)
    path = os.environ.get("MVRT_DENOISE_QUALITY_OUT")
    if path:
        with open(path, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")
