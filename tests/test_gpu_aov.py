"""First-hit feature buffers (mvrt_pt_set_aovs: MVRT_AOV_ALBEDO, MVRT_AOV_NORMAL_DEPTH) on the GPU against buffers computed from oracle primitives alone
(tests/aov_expected.py; its recipe is pinned to the oracle's path tracer by tests/test_aov_cpu.py).  Every comparison is bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import common
import aov_expected as A
from common import GOLDEN, bunny_tris, position_colors, probe_camera
from fixtures import hdr, mv, O  # noqa: F401 (fixtures)
from voxel_mesh_app import read_png_rgba, write_reader_obj

pytestmark = pytest.mark.gpu

OFFSETS = [(6, 4, 6), (-6, -4, -6), (-2.5, 1.5, -2.0)]


@pytest.fixture(scope="module")
def scene(O):
    tris = bunny_tris()
    cols, emis = position_colors(tris)
    sc = O.build_scene_from_triangles(tris, 256, cols, emis)
    assert sc.has_emission == 1
    return sc


def make_pt(mv, sc, w, h, hdr, tile=(0, 1), aovs=True, upload=True, embedded=True, has_emission=None, attrs=None):
    rgba, hw, hh = hdr
    pt = mv.PathTracer()
    pt.setup(None)
    pt.set_tile(*tile)
    if aovs:
        pt.set_aovs(True)
    pt.resizeFrameBufferIfNeeded(None, w, h)
    pt.loadHDRIPixels(None, rgba, hw, hh, rgba, hw, hh)
    if upload:
        pt.m_intersectorOctreeGPU.upload(sc.nodes, sc.attrs if attrs is None else attrs, sc.origin, sc.dps, sc.grid_res, sc.has_emission if has_emission is None else has_emission,
                                         embeddedMask=embedded)
    return pt


def read_aovs(pt, n):
    return pt.read_aov(pt.AOV_ALBEDO)[:n], pt.read_aov(pt.AOV_NORMAL_DEPTH)[:n]


def assert_aovs(pt, exp, what=""):
    n = exp.W * exp.H
    a, nd = read_aovs(pt, n)
    bad = np.nonzero((a != exp.albedo).any(1) | (nd != exp.normal_depth).any(1))[0]
    assert len(bad) == 0, "%s: %d pixels differ, first %s: albedo %s vs %s, normal/depth %s vs %s" % (what, len(bad), bad[:5], a[bad[:2]], exp.albedo[bad[:2]], nd[bad[:2]],
                                                                                                   exp.normal_depth[bad[:2]])
    assert np.array_equal(a, exp.albedo) and np.array_equal(nd, exp.normal_depth)
    # the padding of the owned-pixel layout stays zero
    assert not pt.read_aov(pt.AOV_ALBEDO)[n:].any() and not pt.read_aov(pt.AOV_NORMAL_DEPTH)[n:].any()


# ---- 1. parity ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,iters", [(128, 72, 2), (100, 37, 1)])
def test_feature_buffers_bit_exact(mv, O, scene, hdr, w, h, iters):
    """both buffers == expected for three cameras (thin lens on); in the same run the frame buffer and the per-sample radiance == the oracle's render_pt: switching
    the feature buffers on perturbs nothing.  The inputs are checked too, so that the test cannot pass empty: >= 5 % of each frame's samples hit, >= 50 pixels are
    partly covered (some but not all 16 samples hit), and over the three cameras all six axis normals occur."""
    rgba, hw, hh = hdr
    Hd = O.HDRI(rgba, hw, hh, rgba, hw, hh, math_mode=1)
    normals = set()
    for off in OFFSETS:
        cam = probe_camera(scene.origin, scene.dps, 256, focus=9.0, lens_r=0.05, offset=off)
        pt = make_pt(mv, scene, w, h, hdr)
        exp = A.Expected(O, scene, w, h)
        fb = np.zeros((w * h, 4), np.float32)
        for it in range(iters):
            pt.step(None, cam)
            fb, sl, _ = scene.render_pt(Hd, cam, w, h, it, math_mode=1, fb=fb, want_samples=True, threads=8)
            assert np.array_equal(pt.sample_radiance()[: w * h * 16], sl), (off, it)
            hit, normal = exp.step(cam)
            share, partly, seen = A.frame_statistics(hit, normal)
            print("camera %s %dx%d iteration %d: %.1f %% of the samples hit, %d partly covered pixels, normals %s" % (off, w, h, it, 100 * share, partly, sorted(seen)))
            assert share >= 0.05 and partly >= 50
            normals |= seen
        assert np.array_equal(pt.read_framebuffer()[: w * h], fb), off
        assert_aovs(pt, exp, "camera %s" % (off,))
        # the hit count is consistent with the frame buffer's sample count
        assert (pt.read_aov(pt.AOV_ALBEDO)[: w * h, 3] <= pt.read_framebuffer()[: w * h, 3]).all()
    assert normals == {(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)}


# ---- 2. order under batching ----------------------------------------------------------------------------------------------------------------------
def test_feature_buffers_keep_step_order_under_batching_and_pipelining(mv, O, scene, hdr):
    """8 steps with a camera that moves every step: merged steps, pipelined passes and sibling passes (the defaults) and one step per pass on the caller's
    stream give the buffers of a step-by-step accumulation, bit for bit"""
    w, h, iters = 64, 40, 8
    cams = [probe_camera(scene.origin, scene.dps, 256, focus=9.0 + 0.1 * i, lens_r=0.02 * i, offset=(6 - 0.2 * i, 4, 6 + 0.1 * i)) for i in range(iters)]
    exp = A.Expected(O, scene, w, h)
    for c in cams:
        exp.step(c)
    assert len(np.unique(exp.albedo[:, 3])) > 8  # partial coverage: the order of additions matters
    for serial in (False, True):
        pt = make_pt(mv, scene, w, h, hdr)
        if serial:
            pt.set_batch_steps(1)
            pt.set_pipeline_depth(1)
        for c in cams:
            pt.step(None, c)
        assert pt.getSteps() == iters
        assert_aovs(pt, exp, "serial" if serial else "default batching")
        assert (pt.read_framebuffer()[: w * h, 3] == 16 * iters).all()


# ---- 3. octree flavours ---------------------------------------------------------------------------------------------------------------------------
def test_feature_buffers_of_every_octree_flavour(mv, O, scene, hdr):
    """embedded upload (nVoxelsPSum walk with the top table), plain upload (masks in the nodes), an octree built by the library (cell index) and a tree-flavour
    build (the traversal reports the voxel index): the same frame, each against the expected buffers of the matching oracle scene"""
    w, h = 96, 54
    cam = probe_camera(scene.origin, scene.dps, 256, focus=9.0, lens_r=0.05)
    tris = bunny_tris()
    cols, emis = position_colors(tris)
    exp = A.Expected(O, scene, w, h)
    exp.step(cam)
    assert exp.albedo[:, 3].sum() > 0.05 * w * h * 16
    plain = O.Scene(O.build_octree(scene.morton, 256, dag=False, embed=False), scene.attrs, scene.origin, scene.dps, 256, scene.has_emission, embedded=False)
    exp_plain = A.Expected(O, plain, w, h)
    exp_plain.step(cam)

    pt = make_pt(mv, scene, w, h, hdr)
    pt.step(None, cam)
    assert_aovs(pt, exp, "embedded upload")

    pt = make_pt(mv, plain, w, h, hdr, embedded=False)
    pt.step(None, cam)
    assert_aovs(pt, exp_plain, "plain upload")

    I = mv.IntersectorOctreeGPU
    for flags, name in ((0, "library build"), (I.BUILD_NO_DAG | I.BUILD_NO_EMBEDDED_MASK, "tree flavour")):
        pt = make_pt(mv, scene, w, h, hdr, upload=False)
        pt.m_intersectorOctreeGPU.build(tris.reshape(-1, 3), cols.reshape(-1, 3), emis.reshape(-1, 3), None, scene.origin, scene.dps, 256, flags=flags)
        assert pt.m_intersectorOctreeGPU.info().numberOfVoxels == len(scene.attrs)
        pt.step(None, cam)
        assert_aovs(pt, exp, name)


# ---- 4. tiles ---------------------------------------------------------------------------------------------------------------------------------------
def test_feature_buffers_of_tile_shares_assemble_to_the_frame(mv, O, scene, hdr):
    """3 tile shares at 200 x 113: each buffer gathered rank-major and assembled on the device == the 1-tile buffer == expected"""
    from massivevoxelraytracing_amd import tiles
    w, h, n = 200, 113, 3
    cam = probe_camera(scene.origin, scene.dps, 256, focus=9.0, lens_r=0.05)
    exp = A.Expected(O, scene, w, h)
    hit, _ = exp.step(cam)
    assert hit.mean() >= 0.05
    full = make_pt(mv, scene, w, h, hdr)
    full.step(None, cam)
    assert_aovs(full, exp, "one tile")
    owned = tiles.owned_pixels(w, h, n)
    shares = []
    for r in range(n):
        pt = make_pt(mv, scene, w, h, hdr, tile=(r, n))
        assert pt.owned_pixels() == owned
        pt.step(None, cam)
        shares.append(pt)
    for which, want in ((full.AOV_ALBEDO, exp.albedo), (full.AOV_NORMAL_DEPTH, exp.normal_depth)):
        d_g = mv.DeviceArray((n, owned, 4), np.float32)
        for r, pt in enumerate(shares):
            pt.join(None)
            mv.memcpy_d2d(d_g.ptr + r * owned * 16, pt.aov_dev(which), owned * 16)  # the buffers have the frame buffer's stride
        d_f = mv.DeviceArray((w * h, 4), np.float32)
        mv.assemble_tiles(d_g, n, owned, w, h, d_f)
        mv.synchronize()
        got = d_f.to_host()
        assert np.array_equal(got, full.read_aov(which)[: w * h])
        assert np.array_equal(got, want)
        assert np.array_equal(tiles.assemble(np.stack([pt.read_aov(which) for pt in shares]), w, h), want)


# ---- 5. independence --------------------------------------------------------------------------------------------------------------------------------
def test_feature_buffers_do_not_depend_on_lighting_emission_or_hints(mv, O, scene, hdr):
    w, h = 64, 40
    cam = probe_camera(scene.origin, scene.dps, 256, focus=9.0, lens_r=0.05)
    exp = A.Expected(O, scene, w, h)
    exp.step(cam)
    exp.step(cam)
    dark = scene.attrs.copy()
    dark[:, 4:8] = 0
    for name in ("as it is", "HDRI scale 0", "no emission", "origin hints off"):
        pt = make_pt(mv, scene, w, h, hdr, attrs=dark if name == "no emission" else None, has_emission=0 if name == "no emission" else None)
        if name == "HDRI scale 0":
            pt.set_hdri_scale(0.0)
        if name == "origin hints off":
            pt.set_origin_hints(False)
        pt.step(None, cam)
        pt.step(None, cam)
        assert_aovs(pt, exp, name)


# ---- 6. edits between steps -------------------------------------------------------------------------------------------------------------------------
def test_an_edit_between_steps_recolours_the_second_step_only(mv, O, hdr):
    """scene through updateScene; step; re-colour voxels the first step saw (an attribute-only edit_voxels); step: the first step's albedo uses the old colours, the
    second the new ones -- the edit waits for the steps in flight"""
    tris = bunny_tris()
    cols, emis = position_colors(tris)
    res, w, h = 128, 64, 40
    old = O.build_scene_from_triangles(tris, res, cols, emis)
    cam = probe_camera(old.origin, old.dps, res, focus=9.0, lens_r=0.05)
    pt = make_pt(mv, old, w, h, hdr, upload=False)
    pt.updateScene(tris.reshape(-1, 3), cols.reshape(-1, 3), emis.reshape(-1, 3), None, old.origin, old.dps, res)
    assert pt.m_intersectorOctreeGPU.info().numberOfVoxels == len(old.attrs)
    exp = A.Expected(O, old, w, h)
    pt.step(None, cam)
    exp.step(cam)
    ro, rd = A.primary_rays(O, cam, w, h, 0)
    first = old.trace(ro, rd, threads=8)
    seen = np.unique(first["vIndex"][first["t"] != O.MAX_FLOAT])[::3]
    assert len(seen) > 300
    attrs = old.attrs.copy()
    attrs[seen, 0:3] = 255 - attrs[seen, 0:3]
    m = old.morton[seen]
    xyz = np.zeros((len(seen), 3), np.uint32)
    for b in range(21):
        for a in range(3):
            xyz[:, a] |= (((m >> np.uint64(3 * b + a)) & np.uint64(1)).astype(np.uint32) << np.uint32(b))
    pt.m_intersectorOctreeGPU.edit_voxels(xyz, attrs[seen])
    new = O.Scene(old.nodes, attrs, old.origin, old.dps, res, old.has_emission)
    before = exp.albedo.copy()
    exp.sc = new
    pt.step(None, cam)
    exp.step(cam)
    assert_aovs(pt, exp, "old colours, then new")
    unedited = A.Expected(O, old, w, h)
    unedited.albedo, unedited.steps = before, 1
    unedited.step(cam)
    assert not np.array_equal(unedited.albedo, exp.albedo)  # the edit is visible in the second step


# ---- 7. contract ------------------------------------------------------------------------------------------------------------------------------------
def test_feature_buffer_contract(mv, O, scene, hdr):
    w, h = 64, 40
    n = w * h
    cam = probe_camera(scene.origin, scene.dps, 256, focus=9.0, lens_r=0.05)
    exp = A.Expected(O, scene, w, h)
    exp.step(cam)
    pt = make_pt(mv, scene, w, h, hdr, aovs=False)
    # off by default
    assert pt.aov_dev(pt.AOV_ALBEDO) is None and pt.aov_dev(pt.AOV_NORMAL_DEPTH) is None
    with pytest.raises(mv.MvrtError, match="mvrt_pt_set_aovs"):
        pt.read_aov(pt.AOV_ALBEDO)
    pt.step(None, cam)
    want_fb = pt.read_framebuffer()
    # on after a step: refused, nothing changes
    with pytest.raises(mv.MvrtError, match="clear"):
        pt.set_aovs(True)
    assert pt.aov_dev(pt.AOV_ALBEDO) is None and pt.getSteps() == 1
    assert np.array_equal(pt.read_framebuffer(), want_fb)
    pt.step(None, cam)  # (still a working handle)
    # ... works after a clear
    pt.clearFrameBuffer(None)
    pt.set_aovs(True)
    assert pt.aov_dev(pt.AOV_ALBEDO) and pt.aov_dev(pt.AOV_NORMAL_DEPTH) and pt.aov_dev(pt.AOV_ALBEDO) != pt.aov_dev(pt.AOV_NORMAL_DEPTH)
    assert not pt.read_aov(pt.AOV_ALBEDO).any() and not pt.read_aov(pt.AOV_NORMAL_DEPTH).any()
    assert pt.aov_dev(2) is None
    with pytest.raises(mv.MvrtError, match="MVRT_AOV_ALBEDO"):
        pt.read_aov(2)
    pt.step(None, cam)
    assert_aovs(pt, exp, "switched on after a clear")
    assert np.array_equal(pt.read_framebuffer(), want_fb)
    with pytest.raises(mv.MvrtError, match="clear"):
        pt.set_aovs(False)  # off while steps are accumulated: refused as well
    # clear zeroes them with the frame buffer
    pt.clearFrameBuffer(None)
    assert not pt.read_aov(pt.AOV_ALBEDO).any() and not pt.read_aov(pt.AOV_NORMAL_DEPTH).any()
    pt.step(None, cam)
    assert_aovs(pt, exp, "after a clear")
    # resize reallocates (and clears)
    pt.resizeFrameBufferIfNeeded(None, 100, 37)
    assert pt.owned_pixels() == 3840 and pt.read_aov(pt.AOV_ALBEDO).shape == (3840, 4) and not pt.read_aov(pt.AOV_NORMAL_DEPTH).any()
    pt.resizeFrameBufferIfNeeded(None, w, h)
    pt.step(None, cam)
    assert_aovs(pt, exp, "after two resizes")
    # a reallocation that fails: no frame, no feature buffer; a later resize recovers
    pt.clearFrameBuffer(None)
    pt.set_test_free_bytes(int(n * 16 * 190 * 0.5))
    with pytest.raises(mv.MvrtError, match="mvrt_pt_set_tile"):
        pt.set_pipeline_depth(2)
    assert pt.aov_dev(pt.AOV_ALBEDO) is None and pt.framebuffer_dev() is None
    with pytest.raises(mv.MvrtError, match="no frame buffer"):
        pt.read_aov(pt.AOV_ALBEDO)
    with pytest.raises(mv.MvrtError, match="no frame buffer"):
        pt.step(None, cam)
    with pytest.raises(mv.MvrtError):
        pt.resizeFrameBufferIfNeeded(None, w, h)
    pt.set_test_free_bytes(0)
    pt.resizeFrameBufferIfNeeded(None, w, h)
    pt.step(None, cam)
    assert_aovs(pt, exp, "after a failed reallocation and a resize")
    assert np.array_equal(pt.read_framebuffer(), want_fb)
    # off again: pointers gone, the frame renders as before
    pt.clearFrameBuffer(None)
    pt.set_aovs(False)
    assert pt.aov_dev(pt.AOV_ALBEDO) is None
    pt.step(None, cam)
    assert np.array_equal(pt.read_framebuffer(), want_fb)
    # set_tile releases them with the frame buffer
    pt.clearFrameBuffer(None)
    pt.set_aovs(True)
    pt.set_tile(0, 1)
    assert pt.aov_dev(pt.AOV_ALBEDO) is None
    pt.resizeFrameBufferIfNeeded(None, w, h)
    pt.step(None, cam)
    assert_aovs(pt, exp, "after set_tile")


def test_profiling_counts_the_feature_kernels_as_other(mv, O, scene, hdr):
    """mvrt_pt_set_profiling: the two new launches are timed under 'other' (in totalKernelMs); the counters of mvrt_pt_stats and the number of traversal launches
    are those of a run without feature buffers"""
    w, h = 64, 40
    cam = probe_camera(scene.origin, scene.dps, 256, focus=9.0, lens_r=0.05)
    stats = []
    for on in (False, True):
        pt = make_pt(mv, scene, w, h, hdr, aovs=on)
        pt.set_profiling(True)
        pt.step(None, cam)
        stats.append(pt.stats())
    for k in ("samples", "rays", "shadowRays", "descents", "shadowDescents", "hits", "traceLaunches"):
        assert stats[0][k] == stats[1][k], k
    for s in stats:
        assert s["totalKernelMs"] >= s["traceKernelMs"] + s["shadeKernelMs"] > 0


# ---- 8. the batch driver ----------------------------------------------------------------------------------------------------------------------------
def test_batch_driver_writes_the_feature_images(tmp_path, O):
    """rtcamp_batch --aov: <frame>_albedo and <frame>_normal beside each frame == the bytes computed from the expected buffers with the documented encoding; PPM and PNG"""
    from massivevoxelraytracing_amd import build as b
    exe = b.build_apps(verbose=False)
    tris = bunny_tris()
    obj = tmp_path / "bunny.obj"
    write_reader_obj(obj, tris)
    hdr_file = os.path.join(GOLDEN, "monks_forest_s.hdr")
    W, H, steps = 96, 54, 2
    v = tris.reshape(-1, 3)
    for png in (False, True):
        out = tmp_path / ("png" if png else "ppm")
        os.mkdir(out)
        subprocess.check_call([exe, str(obj), hdr_file, str(out), "--frames", "8", "--frame-range", "5", "6", "--size", str(W), str(H), "--res", "64", "256", "--steps", str(steps),
                               "--dump-cameras", "--aov"] + (["--png"] if png else []))
        lines = open(out / "005.camera.txt").read().split("\n")
        view = np.array([float.fromhex(t) for t in lines[0].split()], np.float32)
        proj = np.array([float.fromhex(t) for t in lines[1].split()], np.float32)
        t = lines[2].split()
        focus, lens_r, ox, oy, oz, dps = (float.fromhex(x) for x in t[:6])
        sc = O.build_scene_from_triangles(tris, int(t[6]), np.ones_like(v).reshape(-1, 9), None, origin=np.array([ox, oy, oz], np.float32), dps=np.float32(dps))
        cam = O.camera_from_matrices(view, proj, focus, lens_r)
        exp = A.Expected(O, sc, W, H)
        for _ in range(steps):
            hit, _n = exp.step(cam)
        assert hit.mean() > 0.05
        samples = np.full(W * H, 16.0 * steps, np.float32)
        for name, want in (("albedo", A.encode_albedo(exp.albedo, samples)), ("normal", A.encode_normal(exp.normal_depth, samples))):
            if png:
                img = read_png_rgba(out / ("005_%s.png" % name)).reshape(H * W, 4)
                assert (img[:, 3] == 255).all()
                got = img[:, :3]
            else:
                ppm = open(out / ("005_%s.ppm" % name), "rb").read()
                got = np.frombuffer(ppm[len(b"P6\n%d %d\n255\n" % (W, H)):], np.uint8).reshape(H * W, 3)
            assert np.array_equal(got, want), (name, png)
            assert len(np.unique(got)) > 3
        assert os.path.exists(out / ("005.png" if png else "005.ppm"))


def test_cpp_mirror_feature_buffer_members(tmp_path):
    """tests/cpp/aov_usage.cpp on the header-only mirror: setAOVs before the frame exists, the two views sized like m_frameBufferF32, a caller's own device read after
    join == mvrt_pt_read_aov, views gone after setAOVs( false ) and after setTile"""
    import shutil
    import massivevoxelraytracing_amd as mv
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, libdir = common.compile_usage(tmp_path, "aov_usage")
    shutil.copy(os.path.join(GOLDEN, "monks_forest_s.hdr"), tmp_path / "monks_forest_s.hdr")
    out = subprocess.check_output([str(exe), "run"], cwd=tmp_path, timeout=300).decode()
    print(out)
    assert "views 1 1 bytes %d %d" % (64 * 36 * 16, 64 * 36 * 16) in out
    assert " same 1" in out and "off 1 1 dev 1" in out and "tile 1 1 1" in out
