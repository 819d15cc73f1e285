"""GPU parity tests (run with -m gpu on the MI355X box): the HIP path, called through the C-ABI,
against the CPU oracle on the same inputs.  Bars: bit-exact for (t, nMajor, vIndex), descents,
compaction indices, per-sample radiance, frame buffers and resolved bytes (the oracle runs in
mathMode 1 = the shared deterministic transcendental set, see include/mvrt_detmath.h)."""
import numpy as np
import pytest

from common import bunny_tris, golden, position_colors, probe_camera
from fixtures import bunny256, hdr, load, O  # noqa: F401 (fixtures)
from rays import assert_hits_equal, make_pt, random_rays, secondary_like_rays, upload

pytestmark = pytest.mark.gpu

G = golden()


@pytest.fixture(scope="module")
def mv():
    m = load()
    assert m.device_count() >= 1
    print("device:", m.device_name())
    return m


@pytest.fixture(scope="module")
def bunny256_color(O):
    tris = bunny_tris()
    cols, emis = position_colors(tris)
    sc = O.build_scene_from_triangles(tris, 256, cols, emis)
    assert sc.has_emission == 1
    return sc


def test_trace_batch_bit_exact(mv, O, bunny256):
    svo = upload(mv, bunny256)
    ro, rd = random_rays(bunny256, 200_000, 7)
    sh = (np.arange(len(ro)) % 3 == 0).astype(np.uint8)
    want = bunny256.trace(ro, rd, sh, threads=8, want_descents=True)
    got = svo.intersect(ro, rd, sh, want_descents=True)
    assert_hits_equal(want, got)
    assert (got["vIndex"][sh == 1] == 0).all()  # shadow rays never accumulate vIndex
    assert (want["t"] != O.MAX_FLOAT).sum() > 10000


@pytest.mark.parametrize("res", [256, 1024])
def test_start_below_the_root_gives_the_results_of_the_walk_from_the_root(mv, O, bunny256, res):
    """mvrt_trace_batch_hinted: every output -- descents included -- equals the oracle's (which starts at the root like the reference) for ANY
    valid hint: the voxel the ray starts on (what the path tracer passes), a voxel somewhere else entirely, no hint; 256^3: the prefix tables reach
    the hint's last level; 1024^3: two levels below them come from the children array"""
    sc = bunny256 if res == 256 else O.build_scene_from_triangles(bunny_tris(), res)
    svo = upload(mv, sc)
    ro0, rd0 = random_rays(sc, 120_000, 21)
    prim = svo.intersect(ro0, rd0, want_descents=True)
    ro, rd, hint = secondary_like_rays(sc, ro0, rd0, prim, 22)
    assert len(ro) > 5000
    rng = np.random.default_rng(23)
    sh = (rng.random(len(ro)) < 0.4).astype(np.uint8)
    want = sc.trace(ro, rd, sh, threads=8, want_descents=True)
    assert_hits_equal(want, svo.intersect_hinted(ro, rd, hint, sh))          # the voxel the ray starts on
    wild = sc.morton[rng.integers(0, len(sc.morton), len(ro))].astype(np.uint64)
    assert_hits_equal(want, svo.intersect_hinted(ro, rd, wild, sh))          # any voxel that exists
    mixed = np.where(rng.random(len(ro)) < 0.5, hint, np.uint64(0xFFFFFFFFFFFFFFFF))
    assert_hits_equal(want, svo.intersect_hinted(ro, rd, mixed, sh))         # half of the rays unhinted
    # rays from outside / inside / axis-parallel (the irregular path) with hints they have nothing to do with
    wild0 = sc.morton[rng.integers(0, len(sc.morton), len(ro0))].astype(np.uint64)
    assert_hits_equal(sc.trace(ro0, rd0, None, threads=8, want_descents=True), svo.intersect_hinted(ro0, rd0, wild0))
    # the hinted walk really skips levels: with the right hint most secondary rays start at least 5 levels down -- visible in nothing but time,
    # so only sanity-check the premise here: the hint's voxel contains (or touches) the origin
    lo, _ = sc.bounds()
    cell = np.floor((ro - lo) / np.float32(sc.dps)).astype(np.int64)
    hx = np.zeros((len(hint), 3), np.int64)
    for b in range(21):
        for a in range(3):
            hx[:, a] |= ((hint >> np.uint64(3 * b + a)) & np.uint64(1)).astype(np.int64) << b
    assert (np.abs(cell - hx).max(1) <= 1).mean() > 0.99


def test_trace_empty_and_ragged_batches(mv, O, bunny256):
    svo = upload(mv, bunny256)
    assert len(svo.intersect(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))["t"]) == 0
    for n in (1, 63, 64, 65, 257):
        ro, rd = random_rays(bunny256, n + 400, n)
        ro, rd = ro[:n], rd[:n]
        assert_hits_equal(bunny256.trace(ro, rd, want_descents=True), svo.intersect(ro, rd, want_descents=True))


def test_trace_non_embedded_variant(mv, O, bunny256):
    """mask fetched from the node (voxCommon.hpp:353-356) on a non-DAG tree: same hits as the DAG"""
    nodes = O.build_octree(bunny256.morton, 256, dag=False, embed=False)
    plain = O.Scene(nodes, bunny256.attrs, bunny256.origin, bunny256.dps, 256, embedded=False)
    svo = upload(mv, plain, embedded=False)
    ro, rd = random_rays(bunny256, 50_000, 11)
    want = bunny256.trace(ro, rd, want_descents=True)
    assert_hits_equal(plain.trace(ro, rd, want_descents=True), want)
    assert_hits_equal(want, svo.intersect(ro, rd, want_descents=True))


def test_uploaded_octree_with_non_canonical_psum_gives_the_stored_sums(mv, O, bunny256):
    """an uploaded octree may carry any nVoxelsPSum -- buildOctreeNaive leaves them zero (IntersectorOctree.hpp:195) and the reference's
    traversal then reports vIndex 0.  The library must sum what is STORED (no popcount shortcut on the last level) for such nodes."""
    nodes = bunny256.nodes.copy()
    nodes["psum"][:] = 0
    sc = O.Scene(nodes, bunny256.attrs, bunny256.origin, bunny256.dps, 256)
    svo = upload(mv, sc)
    ro, rd = random_rays(bunny256, 30_000, 31)
    want = sc.trace(ro, rd, threads=8, want_descents=True)
    got = svo.intersect(ro, rd, want_descents=True)
    assert_hits_equal(want, got)
    assert (got["vIndex"] == 0).all() and (want["t"] != O.MAX_FLOAT).sum() > 1000
    # ... and arbitrary values: a constant 3 per child gives 3 * levels
    nodes["psum"][:] = 3
    sc3 = O.Scene(nodes, bunny256.attrs, bunny256.origin, bunny256.dps, 256)
    got3 = upload(mv, sc3).intersect(ro, rd)
    hit = got3["t"] != O.MAX_FLOAT
    assert (got3["vIndex"][hit] == 24).all()
    assert_hits_equal(sc3.trace(ro, rd, threads=8), got3)


def test_render_primary_golden_and_oracle(mv, O, bunny256):
    svo = upload(mv, bunny256)
    cam = probe_camera(bunny256.origin, bunny256.dps, 256)
    got = svo.render(cam, 1920, 1080)
    g = G["bunny"]["256"]["primary_1080p"]
    hit = got["t"] != O.MAX_FLOAT
    nm = got["nMajor"][hit]
    assert int(hit.sum()) == g["hits"]
    assert [int((nm == k).sum()) for k in (0, 1, 2)] == g["nMajor_z_x_y"]
    assert int(got["vIndex"][hit].astype(np.uint64).sum()) == g["sum_vIndex"]
    want = bunny256.render_primary(cam, 1920, 1080, threads=8)
    assert_hits_equal(want, got)
    assert np.array_equal(want["rgba"], got["rgba"])
    small = svo.render(cam, 256, 144, want_hits=False)
    assert int(small["rgba"].astype(np.uint64).sum()) == G["render_normals_256x144_bytesum"]


def test_render_vertex_colors(mv, O, bunny256_color):
    svo = upload(mv, bunny256_color)
    cam = probe_camera(bunny256_color.origin, bunny256_color.dps, 256)
    got = svo.render(cam, 333, 177, showVertexColor=True)  # not a multiple of 64
    want = bunny256_color.render_primary(cam, 333, 177, show_vertex_color=True, threads=8)
    assert np.array_equal(want["rgba"], got["rgba"])
    assert_hits_equal(want, got)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 255, 256, 257, 1000, 1023, 1024, 1025, 65536, 1_000_003, 1_048_576, 1_048_577, 5_000_011])  # (> 4096 blocks: several scan tiles)
def test_compaction_indices_bit_exact(mv, O, n):
    rng = np.random.default_rng(n)
    for density in (0.0, 0.13, 0.9, 1.0):
        keep = (rng.random(n) < density).astype(np.uint8)
        dst_want, src_want = O.compact_indices(keep)
        dst, kept = mv.compact_indices(keep)
        assert kept == len(src_want)
        assert np.array_equal(dst, dst_want)


def test_hdri_tables_bit_exact(mv, O, bunny256, hdr):
    rgba, w, h = hdr
    pt = make_pt(mv, O, bunny256, 64, 64, rgba, w, h)
    H = O.HDRI(rgba, w, h, rgba, w, h, math_mode=1)
    for which in range(7):
        assert np.array_equal(pt.hdri_sat(which, w, h), H.sat(which)), which


@pytest.mark.parametrize("w,h,iters", [(128, 72, 2), (100, 37, 1)])
def test_path_tracer_bit_exact(mv, O, bunny256_color, hdr, w, h, iters):
    rgba, hw, hh = hdr
    sc = bunny256_color
    cam = probe_camera(sc.origin, sc.dps, 256, focus=9.0, lens_r=0.05)
    pt = make_pt(mv, O, sc, w, h, rgba, hw, hh)
    H = O.HDRI(rgba, hw, hh, rgba, hw, hh, math_mode=1)
    fb = np.zeros((w * h, 4), np.float32)
    tot = dict(rays=0, shadowRays=0, descents=0, shadowDescents=0, hits=0, samples=0)
    for it in range(iters):
        pt.step(None, cam)
        fb, sl, cnt = sc.render_pt(H, cam, w, h, it, math_mode=1, fb=fb, want_samples=True, threads=8)
        for k in tot:
            tot[k] += cnt[k]
        got_sl = pt.sample_radiance()[: w * h * 16]
        bad = np.nonzero((got_sl != sl).any(axis=1))[0]
        assert len(bad) == 0, "iteration %d: %d samples differ, first %s: %s vs %s" % (it, len(bad), bad[:5], got_sl[bad[:2]], sl[bad[:2]])
    got = pt.read_framebuffer()[: w * h]
    assert np.array_equal(got, fb)
    assert pt.getSteps() == iters
    st = pt.stats()
    for k in tot:
        assert st[k] == tot[k], (k, st[k], tot[k])
    # resolve
    u8 = pt.toImageAsync(None)
    mv.synchronize()
    assert np.array_equal(u8[: w * h], O.resolve(fb, math_mode=1))
    assert tot["rays"] > tot["samples"]  # secondary rays were traced


@pytest.mark.parametrize("res", [2, 4, 8, 16, 64])
def test_path_tracer_tiny_grids_and_hints_off(mv, O, hdr, res):
    """the start below the root at the sizes where it has nothing (a 2^3 grid: one level, no hint levels) or little to skip, camera OUTSIDE and
    INSIDE the grid; and switched off (every ray from the root like the reference): frames, samples and every counter equal the oracle's"""
    from common import bunny_tris, position_colors
    rgba, hw, hh = hdr
    tris = bunny_tris()
    cols, emis = position_colors(tris)
    sc = O.build_scene_from_triangles(tris, res, cols, emis)
    H = O.HDRI(rgba, hw, hh, rgba, hw, hh, math_mode=1)
    w, h = 64, 40
    lo, hi = sc.bounds()
    inside = scenes_look_at((lo + hi) / 2 + (hi - lo) * np.array([0.11, 0.07, -0.13]), (lo + hi) / 2 + (hi - lo) * np.array([-0.3, 0.1, 0.35]))
    for cam in (probe_camera(sc.origin, sc.dps, res, focus=9.0, lens_r=0.05), inside):
        fb, sl, cnt = sc.render_pt(H, cam, w, h, 0, math_mode=1, want_samples=True, threads=8)
        for hints in (True, False):
            pt = make_pt(mv, O, sc, w, h, rgba, hw, hh)
            pt.set_origin_hints(hints)
            pt.step(None, cam)
            assert np.array_equal(pt.sample_radiance()[: w * h * 16], sl), (res, hints)
            assert np.array_equal(pt.read_framebuffer()[: w * h], fb)
            st = pt.stats()
            for k in cnt:
                assert st[k] == cnt[k], (res, hints, k, st[k], cnt[k])


def scenes_look_at(eye, target):
    from massivevoxelraytracing_amd import scenes
    return scenes.look_at_camera(eye, target, 70.0, float(np.linalg.norm(np.asarray(target) - np.asarray(eye))), 0.01)


def test_path_tracer_no_emission_and_no_hdri(mv, O, bunny256, hdr):
    rgba, hw, hh = hdr
    w, h = 96, 64
    cam = probe_camera(bunny256.origin, bunny256.dps, 256, focus=9.0, lens_r=0.0)
    H = O.HDRI(rgba, hw, hh, rgba, hw, hh, math_mode=1)
    # (a) white bunny, no emissive voxels: no extra rays (voxKernel.cu:721)
    pt = make_pt(mv, O, bunny256, w, h, rgba, hw, hh)
    pt.step(None, cam)
    fb, _, cnt = bunny256.render_pt(H, cam, w, h, 0, math_mode=1, threads=8)
    assert np.array_equal(pt.read_framebuffer()[: w * h], fb)
    assert pt.stats()["rays"] == cnt["rays"]
    # (b) HDRI disabled (m_scale <= 0, renderCommon.hpp:467-470): no shadow rays at all
    pt2 = make_pt(mv, O, bunny256, w, h, rgba, hw, hh, hdri_scale=0.0)
    pt2.step(None, cam)
    H.set_scale(0.0)
    fb2, _, cnt2 = bunny256.render_pt(H, cam, w, h, 0, math_mode=1, threads=8)
    assert np.array_equal(pt2.read_framebuffer()[: w * h], fb2)
    st = pt2.stats()
    assert st["shadowRays"] == 0 == cnt2["shadowRays"] and st["rays"] == cnt2["rays"]


def test_tile_split_reproduces_single_gpu_image(mv, O, bunny256_color, hdr):
    """3 'ranks' on one GPU: owned tiles rendered separately, assembled on the device, equal the 1-rank frame"""
    from massivevoxelraytracing_amd import tiles
    rgba, hw, hh = hdr
    sc = bunny256_color
    w, h, n = 200, 113, 3
    cam = probe_camera(sc.origin, sc.dps, 256, focus=9.0, lens_r=0.05)
    full = make_pt(mv, O, sc, w, h, rgba, hw, hh)
    full.step(None, cam)
    want = full.read_framebuffer()[: w * h]
    owned = tiles.owned_pixels(w, h, n)
    parts = []
    for r in range(n):
        pt = make_pt(mv, O, sc, w, h, rgba, hw, hh, tile=(r, n))
        assert pt.owned_pixels() == owned
        pt.step(None, cam)
        parts.append(pt.read_framebuffer())
    gathered = np.stack(parts)
    assert np.array_equal(tiles.assemble(gathered, w, h), want)
    d_g = mv.DeviceArray.from_host(gathered)
    d_f = mv.DeviceArray((w * h, 4), np.float32)
    mv.assemble_tiles(d_g, n, owned, w, h, d_f)
    mv.synchronize()
    assert np.array_equal(d_f.to_host(), want)


def test_full_hd_frame_properties(mv, O, bunny256_color, hdr):
    """BASELINE frame size (1920x1080, one 16-spp step): size-independent properties + an oracle band"""
    rgba, hw, hh = hdr
    sc = bunny256_color
    w, h = 1920, 1080
    cam = probe_camera(sc.origin, sc.dps, 256, focus=9.0, lens_r=0.05)
    pt = make_pt(mv, O, sc, w, h, rgba, hw, hh)
    pt.step(None, cam)
    fb = pt.read_framebuffer()
    assert np.isfinite(fb).all() and (fb[:, :3] >= 0).all()
    assert (fb[:, 3] == 16.0).all()
    st = pt.stats()
    assert st["samples"] == w * h * 16
    assert st["samples"] <= st["rays"] <= 18 * st["samples"]  # ray budget, voxKernel.cu:675,691-760
    # a band of 8192 pixels through the bunny, bit-exact against the oracle
    H = O.HDRI(rgba, hw, hh, rgba, hw, hh, math_mode=1)
    p0 = 600 * w + 512
    ref = np.zeros((w * h, 4), np.float32)
    sc.render_pt(H, cam, w, h, 0, math_mode=1, fb=ref, pixel_begin=p0, pixel_end=p0 + 8192, threads=8)
    assert np.array_equal(fb[p0:p0 + 8192], ref[p0:p0 + 8192])
    # idempotence of clear + re-render (deterministic accumulation order)
    pt.clearFrameBuffer(None)
    assert pt.getSteps() == 0
    pt.step(None, cam)
    assert np.array_equal(pt.read_framebuffer(), fb)


@pytest.mark.parametrize("depth", [1, 2, 3, 4])
def test_pipelined_steps_keep_accumulation_order(mv, O, bunny256_color, hdr, depth):
    """step() calls in flight on internal streams (pipeline depth 1..4) give the same frame buffer bit for bit"""
    rgba, hw, hh = hdr
    sc = bunny256_color
    w, h, iters = 160, 90, 5
    cam = probe_camera(sc.origin, sc.dps, 256, focus=9.0, lens_r=0.05)
    pt = make_pt(mv, O, sc, w, h, rgba, hw, hh)
    pt.set_pipeline_depth(depth)
    for _ in range(iters):
        pt.step(None, cam)
    got = pt.read_framebuffer()[: w * h]
    H = O.HDRI(rgba, hw, hh, rgba, hw, hh, math_mode=1)
    fb = np.zeros((w * h, 4), np.float32)
    rays = 0
    for it in range(iters):
        fb, _, cnt = sc.render_pt(H, cam, w, h, it, math_mode=1, fb=fb, threads=8)
        rays += cnt["rays"]
    assert np.array_equal(got, fb)
    assert pt.stats()["rays"] == rays
    # clear + one more step after a pipelined burst
    pt.clearFrameBuffer(None)
    pt.step(None, cam)
    one, _, _ = sc.render_pt(H, cam, w, h, 0, math_mode=1, threads=8)
    assert np.array_equal(pt.read_framebuffer()[: w * h], one)


@pytest.mark.parametrize("batch,depth", [(1, 1), (2, 2), (4, 3), (8, 2), (3, 1)])
def test_deferred_batched_steps_with_moving_camera(mv, O, bunny256_color, hdr, batch, depth):
    """step() calls merged into one wavefront pass (batch) and pipelined (depth): every step keeps its own camera and
    iteration index, and the frame buffer equals step-by-step accumulation bit for bit"""
    rgba, hw, hh = hdr
    sc = bunny256_color
    w, h, iters = 96, 54, 7
    cams = [probe_camera(sc.origin, sc.dps, 256, focus=9.0 + 0.1 * i, lens_r=0.02 * i, offset=(6 - 0.2 * i, 4, 6 + 0.1 * i)) for i in range(iters)]
    pt = make_pt(mv, O, sc, w, h, rgba, hw, hh)
    pt.set_batch_steps(batch)
    pt.set_pipeline_depth(depth)
    for c in cams:
        pt.step(None, c)
    assert pt.getSteps() == iters
    got = pt.read_framebuffer()[: w * h]
    H = O.HDRI(rgba, hw, hh, rgba, hw, hh, math_mode=1)
    fb = np.zeros((w * h, 4), np.float32)
    rays = 0
    for it, c in enumerate(cams):
        fb, _, cnt = sc.render_pt(H, c, w, h, it, math_mode=1, fb=fb, threads=8)
        rays += cnt["rays"]
    assert np.array_equal(got, fb)
    assert pt.stats()["rays"] == rays


def test_split_small_passes_is_result_neutral(mv, O, bunny256_color, hdr):
    """a small multi-step pass launched as two sibling passes with half-grid traversal launches (the default) gives the same
    frame buffer and ray counts as one full-grid pass, bit for bit"""
    rgba, hw, hh = hdr
    sc = bunny256_color
    w, h, iters = 192, 108, 6
    cams = [probe_camera(sc.origin, sc.dps, 256, focus=9.0, lens_r=0.03, offset=(6 - 0.3 * i, 4, 6)) for i in range(iters)]
    out = []
    for enable in (True, False):
        pt = make_pt(mv, O, sc, w, h, rgba, hw, hh)
        pt.set_split_small_passes(enable)
        for c in cams:
            pt.step(None, c)
        out.append((pt.read_framebuffer()[: w * h].copy(), pt.stats()["rays"]))
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]
    assert out[0][0][:, 3].min() == 16 * iters


def test_pass_size_follows_the_frame_length_without_changing_results(mv, O, bunny256_color, hdr):
    """Without a batch size the library merges at most HALF of the caller's frame (the steps between two clearFrameBuffer calls) into one pass, so that a frame is
    at least two passes that overlap; the first frame cannot know its length, later ones do.  Frames of 4, 4, 1, 4 and 6 steps with moving cameras: every frame
    equals the oracle's, whatever the pass sizes were."""
    rgba, hw, hh = hdr
    sc = bunny256_color
    w, h = 96, 54
    H = O.HDRI(rgba, hw, hh, rgba, hw, hh, math_mode=1)
    pt = make_pt(mv, O, sc, w, h, rgba, hw, hh)
    for f, n in enumerate((4, 4, 1, 4, 6)):
        cams = [probe_camera(sc.origin, sc.dps, 256, focus=9.0, lens_r=0.02, offset=(6 - 0.2 * i - 0.1 * f, 4, 6)) for i in range(n)]
        pt.clearFrameBuffer(None)
        for c in cams:
            pt.step(None, c)
        got = pt.read_framebuffer()[: w * h].copy()
        fb = np.zeros((w * h, 4), np.float32)
        for it, c in enumerate(cams):
            fb, _, _ = sc.render_pt(H, c, w, h, it, math_mode=1, fb=fb, threads=8)
        assert np.array_equal(got, fb), (f, n)


def test_trace_tie_cases_bit_exact(mv, O, bunny256):
    """rays that produce EXACT ties between mid-plane and exit times (diagonals through lattice points of the octree, dyadic
    origins): the node-visit step orders events lexicographically by (time, axis) -- the reference's min + 'x first, then y' rule --
    and every tie-break must agree with the oracle, descents included"""
    sc = bunny256
    svo = upload(mv, sc)
    lo, hi = sc.bounds()
    ext = np.float32(sc.dps * sc.grid_res)
    rng = np.random.default_rng(3)
    ros, rds = [], []
    dirs = [(1, 1, 1), (1, 1, -1), (1, -1, 1), (-1, 1, 1), (1, 1, 0.5), (1, 0.5, 1), (0.5, 1, 1), (1, 0.5, 0.25), (2, 1, 1), (1, 2, -1), (-1, -1, -1), (1, -1, -0.5)]
    for k in range(6000):
        # a lattice point of the 256^3 grid (or a node corner of a coarser level) inside the volume, approached along a diagonal
        lvl = int(rng.integers(1, 9))
        cell = ext / np.float32(2 ** lvl)
        p = lo + cell * rng.integers(0, 2 ** lvl + 1, size=3).astype(np.float32)
        d = np.array(dirs[k % len(dirs)], np.float32)
        s = np.float32(2 ** int(rng.integers(0, 3)))  # dyadic distance: origin coordinates stay exactly representable relative to the grid
        ros.append((p - d * ext * s).astype(np.float32))
        rds.append(d if k % 3 else d * np.float32(0.5))
    # and the same directions from inside the volume (origin ON lattice planes: S == 0 / negative events)
    for k in range(3000):
        lvl = int(rng.integers(1, 9))
        cell = ext / np.float32(2 ** lvl)
        p = lo + cell * rng.integers(0, 2 ** lvl + 1, size=3).astype(np.float32)
        ros.append(p.astype(np.float32))
        rds.append(np.array(dirs[k % len(dirs)], np.float32))
    ro, rd = np.array(ros, np.float32), np.array(rds, np.float32)
    sh = (np.arange(len(ro)) % 2).astype(np.uint8)
    want = sc.trace(ro, rd, sh, threads=8, want_descents=True)
    got = svo.intersect(ro, rd, sh, want_descents=True)
    assert_hits_equal(want, got)
    assert (want["t"] != O.MAX_FLOAT).sum() > 500


@pytest.mark.parametrize("batch", [1, 3])
def test_path_tracer_compaction_indices_bit_exact(mv, O, bunny256_color, hdr, batch):
    """north_star: 'bit-exact for ... compaction indices'.  The path tracer's own compaction (survivor counts from the traversal's result
    stores, scan, ballot rank in the shade kernel) must place the survivors of every stage exactly where StreamCompaction::filter
    (StreamCompaction.hpp:87-184) would: slot j holds the j-th surviving sample in ascending sample order.  The oracle says how many of its
    own rays each sample's path hit, i.e. through how many stages it survives."""
    rgba, hw, hh = hdr
    sc = bunny256_color
    w, h = 150, 85  # W*H not a multiple of 256
    cams = [probe_camera(sc.origin, sc.dps, 256, focus=9.0, lens_r=0.03, offset=(6 - 0.4 * i, 4, 6)) for i in range(batch)]
    pt = make_pt(mv, O, sc, w, h, rgba, hw, hh)
    pt.set_batch_steps(batch)
    pt.set_debug_capture(True)
    for c in cams:
        pt.step(None, c)
    H = O.HDRI(rgba, hw, hh, rgba, hw, hh, math_mode=1)
    hits = np.zeros((batch, w * h * 16), np.uint8)
    for it, c in enumerate(cams):
        sc.render_pt(H, c, w, h, it, math_mode=1, threads=8, path_hits=hits[it])
    flat = hits.reshape(-1)  # sample id = (step * pixels + pixel) * 16 + spp
    total = 0
    for s in range(8):
        got = pt.debug_stage_survivors(s, batch * w * h * 16)
        assert np.array_equal(got, np.nonzero(flat > s)[0].astype(np.uint32)), s
        total += len(got)
    assert total > 0 and (flat > 1).any()


def test_state_changes_between_deferred_steps(mv, O, bunny256_color, hdr):
    """step() is deferred and batched inside the library, but the reference passes the HDRI and the intersector to the kernel BY VALUE at
    call time (PathTracer.hpp:150-169): a step must render with the state it was issued under.  step; change the HDRI scale and the
    emission scale; step; replace the scene; step -- against the oracle doing the same, and against an unbatched tracer."""
    rgba, hw, hh = hdr
    sc = bunny256_color
    w, h = 96, 54
    cam = probe_camera(sc.origin, sc.dps, 256, focus=9.0, lens_r=0.05)
    plain = O.build_scene_from_triangles(bunny_tris(), 256)
    results = []
    for batch in (8, 1):
        pt = make_pt(mv, O, sc, w, h, rgba, hw, hh)
        pt.set_batch_steps(batch)
        pt.step(None, cam)                       # iteration 0: scale 1.75, emission 7.5
        pt.set_hdri_scale(0.5)
        pt.m_intersectorOctreeGPU.set_emission_scale(2.0)
        pt.step(None, cam)                       # iteration 1: scale 0.5, emission 2
        pt.m_intersectorOctreeGPU.upload(plain.nodes, plain.attrs, plain.origin, plain.dps, 256, plain.has_emission)
        pt.step(None, cam)                       # iteration 2: white bunny without emission
        results.append(pt.read_framebuffer()[: w * h].copy())
    assert np.array_equal(results[0], results[1])
    H = O.HDRI(rgba, hw, hh, rgba, hw, hh, math_mode=1)
    fb, _, _ = sc.render_pt(H, cam, w, h, 0, math_mode=1, threads=8)
    H.set_scale(0.5)
    sc.set_emission_scale(2.0)
    fb, _, _ = sc.render_pt(H, cam, w, h, 1, math_mode=1, fb=fb, threads=8)
    sc.set_emission_scale(7.5)
    fb, _, _ = plain.render_pt(H, cam, w, h, 2, math_mode=1, fb=fb, threads=8)
    assert np.array_equal(results[0], fb)


def test_product_pmj_table_is_the_golden_table(mv):
    """PMJSampler::setup (pmjSampler.hpp:114-144): the PRODUCT's table, read back from the device, has the SHA-256 the survey captured"""
    import hashlib
    pt = mv.PathTracer()
    pt.setup(None)
    t = pt.pmj_table()
    assert t.nbytes == G["pmj_table_bytes"]
    assert hashlib.sha256(t.tobytes()).hexdigest() == G["pmj_table_sha256"]


def test_gpu_frame_within_stated_tolerance_of_reference_host_math(mv, O, bunny256_color, hdr):
    """The stated fp32 tolerance against the REFERENCE's arithmetic, checked on the GPU: the HIP path computes sin / cos / atan2 / pow with
    the deterministic set of include/mvrt_detmath.h, the reference's host build with libm (vectorMath.hpp:93-97; its GPU build with fast
    intrinsics, :86-92).  Against the oracle in mathMode 0 (libm -- the mode the survey's goldens pin) a 4-step, 64-spp frame must agree
    within 1e-3 relative on the mean radiance, most pixels bit for bit, ray count within 1e-3; the resolved 8-bit image within 1 level on
    >= 99 % of the bytes."""
    rgba, hw, hh = hdr
    sc = bunny256_color
    w, h, iters = 192, 108, 4
    cam = probe_camera(sc.origin, sc.dps, 256, focus=9.0, lens_r=0.05)
    pt = make_pt(mv, O, sc, w, h, rgba, hw, hh)
    for _ in range(iters):
        pt.step(None, cam)
    got = pt.read_framebuffer()[: w * h]
    u8 = pt.toImageAsync(None)[: w * h]
    mv.synchronize()
    H0 = O.HDRI(rgba, hw, hh, rgba, hw, hh, math_mode=0)
    ref = np.zeros((w * h, 4), np.float32)
    rays = 0
    for it in range(iters):
        ref, _, cnt = sc.render_pt(H0, cam, w, h, it, math_mode=0, fb=ref, threads=8)
        rays += cnt["rays"]
    mg, mr = got[:, :3].astype(np.float64).mean(0), ref[:, :3].astype(np.float64).mean(0)
    assert np.abs(mg - mr).max() / mr.max() < 1e-3
    assert (got == ref).all(axis=1).mean() > 0.6          # 64 spp: a pixel stays identical only if all 64 paths do
    assert abs(pt.stats()["rays"] - rays) / rays < 1e-3
    ref8 = O.resolve(ref, math_mode=0)
    assert (np.abs(u8[:, :3].astype(np.int32) - ref8[:, :3].astype(np.int32)) <= 1).mean() > 0.99
