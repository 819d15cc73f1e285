"""The environment light on the GPU with maps other than the 64x32 fixture (run with -m gpu): importance tables of maps that take kSatScan through
its chunk carry and kHdriImportance through partial 8x8 blocks, a primary map of another size and none at all, maps with tables that have no total
(all zeros; they select nothing -- include/mvrt.h at mvrt_pt_load_hdri), a map of nothing but f32 denormals, the .hdr file path with two files,
and the argument checks of mvrt_pt_load_hdri.  Bars as in test_gpu_parity.py: bit-exact against the CPU oracle in math mode 1, which
tests/test_hdri_cpu.py pins to a float64 reference for the same maps."""
import numpy as np
import pytest

import hdri_maps as M
from common import bunny_tris, position_colors, probe_camera
from fixtures import mv, O  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

RES, W, H = 64, 64, 40


@pytest.fixture(scope="module")
def bunny64(O):
    tris = bunny_tris()
    cols, emis = position_colors(tris)
    sc = O.build_scene_from_triangles(tris, RES, cols, emis)
    assert sc.has_emission == 1
    return sc


@pytest.fixture(scope="module")
def cams(bunny64):
    """the probe camera outside the grid and one inside it (as test_path_tracer_tiny_grids_and_hints_off)"""
    from massivevoxelraytracing_amd import scenes
    sc = bunny64
    lo, hi = sc.bounds()
    eye = (lo + hi) / 2 + (hi - lo) * np.array([0.11, 0.07, -0.13])
    target = (lo + hi) / 2 + (hi - lo) * np.array([-0.3, 0.1, 0.35])
    inside = scenes.look_at_camera(eye, target, 70.0, float(np.linalg.norm(target - eye)), 0.01)
    return [probe_camera(sc.origin, sc.dps, RES, focus=9.0, lens_r=0.05), inside]


@pytest.fixture(scope="module")
def table_pt(mv):
    """one path tracer for all table loads: a load replaces the map as a whole"""
    pt = mv.PathTracer()
    pt.setup(None)
    return pt


def make_pt(mv, sc, light, primary=None):
    pt = mv.PathTracer()
    pt.setup(None)
    pt.resizeFrameBufferIfNeeded(None, W, H)
    if primary is None:
        pt.loadHDRIPixels(None, *light)
    else:
        pt.loadHDRIPixels(None, *light, *primary)
    pt.m_intersectorOctreeGPU.upload(sc.nodes, sc.attrs, sc.origin, sc.dps, sc.grid_res, sc.has_emission)
    return pt


def frame(pt, cam):
    pt.clearFrameBuffer(None)
    pt.step(None, cam)
    return pt.read_framebuffer()[: W * H].copy()


# sizes: one pixel, one row, one column; partial 8x8 blocks; one short of, exactly and one past a 512-entry scan chunk along x and along y;
# two chunks and a rest; 520x260 and 1030x515: a carry in both directions at once.  Then the maps with zero tables, a huge range, only denormals.
TABLE_CASES = [("noise", w, h) for w, h in [(1, 1), (2, 1), (1, 2), (7, 5), (511, 3), (512, 2), (513, 3), (3, 513), (1025, 2), (2, 1025), (520, 260), (1030, 515)]]
TABLE_CASES += [("black_ground", 520, 260), ("sun", 520, 260), ("denormal_floor", 520, 260), ("all_black", 8, 4)]


@pytest.mark.parametrize("kind,w,h", TABLE_CASES)
def test_hdri_tables_bit_exact(mv, O, table_pt, kind, w, h):
    """all seven tables equal the oracle's.  The denormal-floor map is nothing but f32 denormals (pixels, luminance, lum * sr * wgt): its tables match
    only if kHdriImportance keeps f32 denormals as the oracle's host arithmetic does -- flushed, every table would have no total and be zero."""
    rgba = getattr(M, kind)(w, h)
    table_pt.loadHDRIPixels(None, rgba, w, h)
    Hd = O.HDRI(rgba, w, h, rgba, w, h, math_mode=1)
    for which in range(7):
        want = Hd.sat(which)
        if kind in ("noise", "sun", "denormal_floor") and w * h > 2:
            assert want[-1] == 0xFFFFFFFF  # these have no zero table: a device table of zeros is not hidden by an oracle that agrees
        assert np.array_equal(table_pt.hdri_sat(which, w, h), want), (kind, w, h, which)


def noise2(w, h, seed):
    return (M.noise(w, h, seed), w, h)


PT_CASES = {
    # name: (lighting map, primary map given to the library or None, degenerate)
    "other_primary": (lambda: noise2(520, 260, 1), lambda: noise2(130, 65, 9), False),
    "no_primary": (lambda: noise2(1030, 515, 1), None, False),
    "sun": (lambda: (M.sun(520, 260), 520, 260), "same", False),
    "black_ground": (lambda: (M.black_ground(520, 260), 520, 260), "same", True),
    "all_black": (lambda: (M.all_black(8, 4), 8, 4), "same", True),
    "one_pixel": (lambda: (M.constant(1, 1), 1, 1), "same", True),
}


@pytest.mark.parametrize("name", list(PT_CASES))
def test_path_tracer_bit_exact(mv, O, bunny64, cams, name):
    """one 16-spp step of the emissive bunny at 64^3, 64x40 pixels, from outside and from inside: per-sample radiance, frame buffer and all six
    counters equal the oracle's.  With no primary map the oracle is given the lighting map as its primary -- the documented meaning of NULL.  Maps
    with zero tables (black ground: -y; all black: all seven, at the default scale; one pixel: -x, +y, -y, -z): also every value finite and >= 0,
    and as many shadow rays as the oracle -- a hit whose normal selects a zero table still sends its shadow ray."""
    make_light, make_primary, degenerate = PT_CASES[name]
    light = make_light()
    primary = light if make_primary == "same" else None if make_primary is None else make_primary()
    pt = make_pt(mv, bunny64, light, primary)
    Hd = O.HDRI(*light, *(primary or light), math_mode=1)
    sc = bunny64
    tot = dict(rays=0, shadowRays=0, descents=0, shadowDescents=0, hits=0, samples=0)  # the tracer's counters run on from frame to frame
    for cam in cams:
        fb, sl, cnt = sc.render_pt(Hd, cam, W, H, 0, math_mode=1, want_samples=True, threads=8)
        got = frame(pt, cam)
        got_sl = pt.sample_radiance()[: W * H * 16]
        assert np.array_equal(got_sl, sl), name
        assert np.array_equal(got, fb), name
        st = pt.stats()
        for k in tot:
            tot[k] += cnt[k]
            assert st[k] == tot[k], (name, k, st[k], tot[k])
        assert cnt["shadowRays"] > 0 and cnt["hits"] > 0
        if degenerate:
            assert np.isfinite(got_sl).all() and (got_sl >= 0).all() and np.isfinite(got).all() and (got >= 0).all()
            assert st["shadowRays"] == tot["shadowRays"]


def test_primary_map_of_another_size_is_the_one_looked_up(mv, O, bunny64, cams):
    """the pixels whose 16 primary rays all miss show nothing but the primary map: with a 130x65 primary of other noise every one of them differs
    from the run whose primary is the 520x260 lighting map, and both runs equal the oracle's"""
    sc, cam = bunny64, cams[0]
    light, other = noise2(520, 260, 1), noise2(130, 65, 9)
    hits = np.zeros(W * H * 16, np.uint8)
    want_other, _, _ = sc.render_pt(O.HDRI(*light, *other, math_mode=1), cam, W, H, 0, math_mode=1, threads=8, path_hits=hits)
    want_same, _, _ = sc.render_pt(O.HDRI(*light, *light, math_mode=1), cam, W, H, 0, math_mode=1, threads=8)
    miss = ~hits.reshape(W * H, 16).any(axis=1)
    assert miss.sum() > 200
    got_other = frame(make_pt(mv, sc, light, other), cam)
    got_same = frame(make_pt(mv, sc, light, light), cam)
    assert np.array_equal(got_other, want_other) and np.array_equal(got_same, want_same)
    assert (got_other[miss, :3] != got_same[miss, :3]).any(axis=1).all()
    all_hit = (hits.reshape(W * H, 16) > 0).all(axis=1)  # ... and a pixel whose 16 primary rays all hit never looks the primary map up
    assert all_hit.sum() > 200 and np.array_equal(got_other[all_hit], got_same[all_hit])


def test_load_hdri_from_two_files(mv, O, bunny64, cams, tmp_path):
    """loadHDRI( file, filePrimary ) with a 520x260 lighting map and a 130x65 primary map, written as flat RGBE: the same tables and the same frame
    as loadHDRIPixels with read_rgbe_file's pixels of the two files, and the tables of the oracle for those pixels"""
    files = []
    for name, (rgba, w, h) in (("light.hdr", noise2(520, 260, 1)), ("primary.hdr", noise2(130, 65, 9))):
        p = tmp_path / name
        p.write_bytes(M.encode_rgbe_flat(rgba, w, h))
        files.append(str(p))
    light, primary = mv.read_rgbe_file(files[0]), mv.read_rgbe_file(files[1])
    assert light[1:] == (520, 260) and primary[1:] == (130, 65)
    assert np.abs(light[0] - noise2(520, 260, 1)[0]).max() < 2.0 ** -7  # RGBE keeps 8 bits of the largest channel: the files hold these maps
    a = make_pt(mv, bunny64, light, primary)
    b = mv.PathTracer()
    b.setup(None)
    b.resizeFrameBufferIfNeeded(None, W, H)
    b.loadHDRI(None, files[0], files[1])
    b.m_intersectorOctreeGPU.upload(bunny64.nodes, bunny64.attrs, bunny64.origin, bunny64.dps, bunny64.grid_res, bunny64.has_emission)
    Hd = O.HDRI(*light, *primary, math_mode=1)
    for which in range(7):
        t = b.hdri_sat(which, 520, 260)
        assert np.array_equal(t, a.hdri_sat(which, 520, 260)) and np.array_equal(t, Hd.sat(which)), which
    want, _, _ = bunny64.render_pt(Hd, cams[0], W, H, 0, math_mode=1, threads=8)
    fa, fb = frame(a, cams[0]), frame(b, cams[0])
    assert np.array_equal(fa, fb) and np.array_equal(fb, want)


def test_load_hdri_refuses_bad_sizes_and_keeps_the_map(mv, O, bunny64, cams):
    """a primary map with a non-positive size and a lighting or primary map of 2^31 pixels or more are refused with a message, before a pointer is
    read: the oversize calls pass a ONE-pixel buffer.  The map loaded before stays: same tables, same frame."""
    light = noise2(64, 32, 4)
    pt = make_pt(mv, bunny64, light, light)
    before = frame(pt, cams[0])
    tables = [pt.hdri_sat(i, 64, 32) for i in range(7)]
    one = np.ones((1, 4), np.float32)
    for wp, hp in ((0, 32), (64, 0), (-64, 32), (64, -1), (0, 0)):
        with pytest.raises(mv.MvrtError, match="bad primary image size"):
            pt.loadHDRIPixels(None, *light, light[0], wp, hp)
    for w, h in ((65536, 32768), (32768, 65536), (2 ** 31 - 1, 2), (2 ** 31 - 1, 2 ** 31 - 1)):
        with pytest.raises(mv.MvrtError, match="2\\^31 pixels or more"):
            pt.loadHDRIPixels(None, one, w, h)
        with pytest.raises(mv.MvrtError, match="primary .* 2\\^31 pixels or more"):
            pt.loadHDRIPixels(None, *light, one, w, h)
    assert all(np.array_equal(pt.hdri_sat(i, 64, 32), tables[i]) for i in range(7))
    assert np.array_equal(frame(pt, cams[0]), before)
    want, _, _ = bunny64.render_pt(O.HDRI(*light, *light, math_mode=1), cams[0], W, H, 0, math_mode=1, threads=8)
    assert np.array_equal(before, want)
