"""Octrees of 14 to 21 levels on the GPU against the oracle, bit for bit: builds from voxel lists, synthetic and triangle builds, traces
(t, nMajor, vIndex, descents), the cell-index boundary (built up to 14 levels, the nVoxelsPSum walk above), hints, the device API's level
limit, primary renders, path-tracer steps (the LDS ring wraps twice at 17 levels and more) and edits with 21-bit coordinates.  The scenes
come from tests/deep_scenes.py: clusters on the grid's corners and in its middle plus isolated voxels, and rays aimed at them."""
import ctypes as C
import os

import numpy as np
import pytest

import deep_scenes as D
from edit_model import SET, Model, assert_svo, has_emission
from fixtures import hdr, mv, O  # noqa: F401 (fixtures)
from rays import assert_hits_equal, compile_probe, probe_trace, secondary_like_rays, synthetic_reference

pytestmark = pytest.mark.gpu

THREADS = min(16, len(os.sched_getaffinity(0)))
MAXF = np.float32(3.402823466e38)
NO_HINT = np.uint64(0xFFFFFFFFFFFFFFFF)


def build(mv, s, flags=0, svo=None):
    svo = mv.IntersectorOctreeGPU() if svo is None else svo
    svo.build_voxels(s.xyz, s.attrs, origin=s.origin, dps=s.dps, gridRes=s.res, flags=flags)
    assert svo.info().levels == s.levels
    return svo


def ray_sets(s, seed):
    ro = [s.short_rays(6000, seed)[:2], s.long_rays(6000, seed + 1), s.tie_rays(3000, seed + 2)]
    ro, rd = np.concatenate([r[0] for r in ro]), np.concatenate([r[1] for r in ro])
    sh = (np.arange(len(ro)) % 3 == 0).astype(np.uint8)
    return ro, rd, sh


# ---- 1 + 3: builds from the voxel list and traces, every depth and flavour ---------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("levels", D.DEPTHS)
def test_voxel_list_build_and_trace(mv, O, levels, flags):
    s = D.scene(levels)
    sc = D.oracle_scene(O, s, flags)
    svo = build(mv, s, flags)
    assert_svo(O, svo, sc.morton, sc.attrs, 1, s.res, flags, len(s.xyz), nodes=sc.nodes)
    assert svo.info().flavour == (2 if flags == 3 else int(flags == 2))
    ro, rd, sh = ray_sets(s, 10 * levels + flags)
    want = sc.trace(ro, rd, sh, threads=THREADS, want_descents=True)
    assert (want["t"] != MAXF).sum() > len(ro) // 2
    assert (want["descents"][want["t"] != MAXF] >= levels).all()
    assert_hits_equal(want, svo.intersect(ro, rd, sh, want_descents=True))


@pytest.mark.parametrize("levels", [14, 21])
def test_synthetic_build(mv, O, levels):
    res, n = 1 << levels, 300_000
    svo = mv.IntersectorOctreeGPU()
    svo.build_synthetic(res, n, seed=4321, flags=0)
    morton_w, attrs_w, he = synthetic_reference(O, res, n, 4321)
    nodes_w = O.build_octree(morton_w, res)
    assert svo.info().levels == levels
    assert_svo(O, svo, morton_w, attrs_w, he, res, 0, n, nodes=nodes_w)


def test_read_voxels_gives_the_sorted_unique_input_at_21_bits(mv, O):
    s = D.scene(21)
    svo = build(mv, s)
    xyz, attrs = svo.read_voxels()
    m, a, _ = O.merge_voxels(O.morton_encode_batch(s.xyz), s.attrs)
    assert np.array_equal(xyz, D.decode(m)) and np.array_equal(attrs, a)
    assert (xyz.min(0) == 0).all() and (xyz.max(0) == (1 << 21) - 1).all()
    assert ((xyz >> 20) & 1).any(0).all()


# ---- 2: triangles at 21-bit coordinates ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, 4])
def test_triangle_build_at_2_21(mv, O, flags):
    res = 1 << 21
    dps = np.float32(1.0 / res)
    rng = np.random.default_rng(77)
    base = np.array([0.75, 0.6, 0.875])  # bit 20 set on every axis
    small = base + (rng.random((40, 1, 3)) * 0.002 + rng.random((40, 3, 3)) * 6 / res)
    big = base + np.array([[[0, 0, 0], [150, 3, 10], [4, 120, 30]]]) / res  # a footprint of ~9000 cells: the whole-wave path
    tris = np.concatenate([small, big]).astype(np.float32).reshape(-1, 9)
    cols = rng.random(tris.shape).astype(np.float32)
    emis = np.where(rng.random((len(tris), 1)) < 0.3, rng.random(tris.shape), 0).astype(np.float32)
    origin = np.zeros(3, np.float32)
    svo = mv.IntersectorOctreeGPU()
    svo.build(tris.reshape(-1, 3), cols.reshape(-1, 3), emis.reshape(-1, 3), None, origin, dps, res, flags=flags)
    m, at = O.voxelize(tris, origin, dps, res, cols, emis, six_separating=(flags == 0))
    dumped = len(m)
    m, at, he = O.merge_voxels(m, at)
    xyz = D.decode(m)
    assert (xyz >= (1 << 20)).all() and len(m) > 9000
    assert svo.info().levels == 21
    assert_svo(O, svo, m, at, he, res, 0, dumped)


# ---- 4: the cell-index boundary ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [14, 15])
def test_cell_index_boundary(mv, O, levels):
    """built octrees of up to 14 levels resolve vIndex through the cell index (a 2^30-entry block table at 14 levels), deeper ones and uploads
    through the nVoxelsPSum walk: both give every voxel's Morton rank"""
    s = D.DeepScene(levels, seed=50 + levels)
    rng = np.random.default_rng(levels)
    s.xyz = np.concatenate([s.xyz, rng.integers(0, s.res, size=(40_000, 3)).astype(np.uint32)])
    s.attrs = np.concatenate([s.attrs, rng.integers(0, 256, size=(40_000, 8)).astype(np.uint8)])
    s.morton = np.unique(D.morton(s.xyz))
    sc = D.oracle_scene(O, s)
    built = build(mv, s)
    walked = mv.IntersectorOctreeGPU()
    walked.upload(sc.nodes, sc.attrs, s.origin, s.dps, s.res, sc.has_emission)
    assert walked.info().levels == levels
    block_table = 4 << 30
    if levels == 14:
        assert built.traversal_bytes() >= block_table > walked.traversal_bytes()
    else:
        assert built.traversal_bytes() < block_table and built.traversal_bytes() < 2 * walked.traversal_bytes()
    n = len(sc.morton)
    assert n >= 50_000
    xyz = D.decode(sc.morton).astype(np.float64)
    ro = s.to_world(xyz + np.array([0.5, 1.25, 0.5]))
    rd = np.tile(np.array([0.0, -1.0, 0.0], np.float32), (n, 1))
    ref = sc.trace(ro, rd, threads=THREADS)
    assert (ref["t"] != MAXF).all() and np.array_equal(ref["vIndex"], np.arange(n, dtype=np.uint32))
    for svo in (built, walked):
        got = svo.intersect(ro, rd)
        assert np.array_equal(got["t"], ref["t"]) and np.array_equal(got["vIndex"], ref["vIndex"])


# ---- 5: hints ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [14, 17, 21])
def test_hints(mv, O, levels):
    s = D.scene(levels)
    sc = D.oracle_scene(O, s)
    svo = build(mv, s)
    ro0, rd0 = s.long_rays(20_000, 3 * levels)
    ro1, rd1 = s.short_rays(10_000, 3 * levels + 1)[:2]
    ro0, rd0 = np.concatenate([ro0, ro1]), np.concatenate([rd0, rd1])
    prim = svo.intersect(ro0, rd0, want_descents=True)
    ro, rd, hint = secondary_like_rays(sc, ro0, rd0, prim, 5 * levels)
    assert len(ro) > 10_000
    rng = np.random.default_rng(levels)
    sh = (rng.random(len(ro)) < 0.3).astype(np.uint8)
    want = sc.trace(ro, rd, sh, threads=THREADS, want_descents=True)
    assert_hits_equal(want, svo.intersect_hinted(ro, rd, hint, sh))
    wild = sc.morton[rng.integers(0, len(sc.morton), len(ro))].astype(np.uint64)
    assert_hits_equal(want, svo.intersect_hinted(ro, rd, wild, sh))
    assert_hits_equal(want, svo.intersect_hinted(ro, rd, np.full(len(ro), NO_HINT), sh))


# ---- 6: the device API's level limit ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(mv, tmp_path_factory):
    return compile_probe(tmp_path_factory.mktemp("deep_probe"), [])


@pytest.mark.parametrize("flags", [0, 2])
def test_device_api_at_16_levels(mv, O, probe, flags):
    s = D.scene(16)
    sc = D.oracle_scene(O, s, flags)
    svo = build(mv, s, flags)
    view = svo.device_view()
    assert view.flavour == (1 if flags else 0) and view.levels == 16
    ro, rd, sh = ray_sets(s, 160 + flags)
    lib = svo.intersect(ro, rd, sh, want_descents=True)
    assert_hits_equal(sc.trace(ro, rd, sh, threads=THREADS, want_descents=True), lib)
    for mode in (0, 1):
        got = probe_trace(mv, probe, view, ro, rd, sh, mode)
        for k in ("t", "nMajor", "vIndex", "descents"):
            assert np.array_equal(got[k], lib[k]), (mode, k)
    n = len(sc.attrs)
    col, em, raw, he = mv.DeviceArray((n, 4), np.uint8), mv.DeviceArray((n, 3), np.float32), mv.DeviceArray((n, 3), np.float32), mv.DeviceArray(1, np.uint32)
    assert probe.probe_attrs(C.byref(view), n, col.ptr, em.ptr, raw.ptr, he.ptr) == 0
    assert np.array_equal(col.to_host(), sc.attrs[:, 0:4])
    e = sc.attrs[:, 4:7].astype(np.float32) / np.float32(255)
    assert np.array_equal(raw.to_host(), e) and np.array_equal(em.to_host(), (e * np.float32(view.emissionScale)).astype(np.float32))
    assert he.to_host()[0] == 1


def test_device_view_refuses_17_levels(mv):
    svo = build(mv, D.scene(17))
    with pytest.raises(mv.MvrtError, match="17 levels, the device API supports at most 16"):
        svo.device_view()


# ---- 7: primary render and path tracer -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [15, 21])
def test_render_primary(mv, O, levels):
    s = D.scene(levels)
    sc = D.oracle_scene(O, s)
    svo = build(mv, s)
    cam = s.camera()
    want = sc.render_primary(cam, 128, 96, threads=THREADS)
    got = svo.render(cam, 128, 96)
    assert (want["t"] != MAXF).mean() > 0.04
    assert np.array_equal(got["rgba"], want["rgba"])
    assert_hits_equal(want, got)


def make_pt(mv, hdr, w, h):
    rgba, hw, hh = hdr
    pt = mv.PathTracer()
    pt.setup(None)
    pt.resizeFrameBufferIfNeeded(None, w, h)
    pt.loadHDRIPixels(None, rgba, hw, hh, rgba, hw, hh)
    return pt


def oracle_frames(O, sc, hdr, cam, w, h, steps):
    rgba, hw, hh = hdr
    H = O.HDRI(rgba, hw, hh, rgba, hw, hh, math_mode=1)
    fb = np.zeros((w * h, 4), np.float32)
    out = []
    for it in range(steps):
        fb, _, _ = sc.render_pt(H, cam, w, h, it, math_mode=1, fb=fb, threads=THREADS)
        out.append(fb.copy())
    return out


@pytest.mark.parametrize("levels,flags", [(14, 0), (17, 0), (17, 3), (21, 0)])
def test_path_tracer_steps(mv, O, hdr, levels, flags):
    s = D.scene(levels)
    sc = D.oracle_scene(O, s, flags)
    w, h = 128, 72
    cam = s.camera()
    want = oracle_frames(O, sc, hdr, cam, w, h, 2)
    assert (want[0][:, :3] > 0).any()
    for hints in (True, False):
        pt = make_pt(mv, hdr, w, h)
        pt.set_origin_hints(hints)
        build(mv, s, flags, svo=pt.m_intersectorOctreeGPU)
        for it in range(2):
            pt.step(None, cam)
            assert np.array_equal(pt.read_framebuffer()[: w * h], want[it]), (hints, it)


def test_path_tracer_across_octrees_of_10_and_21_levels(mv, O, hdr):
    """one PathTracer: its spill rows must grow when the octree gets deeper between steps"""
    w, h = 128, 72
    pt = make_pt(mv, hdr, w, h)
    for levels in (10, 21, 10):
        s = D.scene(levels)
        sc = D.oracle_scene(O, s)
        cam = s.camera()
        pt.m_intersectorOctreeGPU.upload(sc.nodes, sc.attrs, s.origin, s.dps, s.res, sc.has_emission)
        assert pt.m_intersectorOctreeGPU.info().levels == levels
        pt.clearFrameBuffer(None)
        pt.step(None, cam)
        assert np.array_equal(pt.read_framebuffer()[: w * h], oracle_frames(O, sc, hdr, cam, w, h, 1)[0]), levels


# ---- 8: edits at 21 levels -------------------------------------------------------------------------------------------------------------------------
def test_edits_at_21_levels(mv, O):
    s = D.scene(21)
    res = s.res
    svo = build(mv, s)
    model = Model(O, s.xyz, s.attrs)
    rng = np.random.default_rng(2121)
    existing = np.array(sorted(model.d), np.uint64)
    pick = D.decode(existing[rng.integers(0, len(existing), 40_000)])
    fresh = rng.integers(0, res, size=(40_000, 3)).astype(np.uint32)
    near = (D.decode(existing[rng.integers(0, len(existing), 10_000)]).astype(np.int64) + rng.integers(-1, 2, (10_000, 3))).clip(0, res - 1)
    corners = np.array([[x, y, z] for x in (0, res - 1) for y in (0, res - 1) for z in (0, res - 1)], np.uint32)
    xyz = np.concatenate([pick, fresh, near.astype(np.uint32), corners, corners])
    xyz = np.concatenate([xyz, xyz[rng.integers(0, len(xyz), 10_000)]])  # repeats: the last one wins
    attrs = rng.integers(0, 256, size=(len(xyz), 8), dtype=np.uint8)
    attrs[rng.random(len(xyz)) >= 0.1, 4:7] = 0
    ops = (rng.random(len(xyz)) < 0.6).astype(np.uint8)
    ops[-len(corners) - 10_000:-10_000] = SET
    assert len(xyz) >= 100_000
    model.apply(O, xyz, attrs, ops)
    svo.edit_voxels(xyz, attrs, ops)
    m, a = model.arrays()
    assert_svo(O, svo, m, a, has_emission(a), res, 0, 0)
    assert np.isin(D.morton(corners), m).all()
    sc = O.Scene(O.build_octree(m, res), a, s.origin, s.dps, res, has_emission(a))
    ro, rd, sh = ray_sets(s, 2122)
    assert_hits_equal(sc.trace(ro, rd, sh, threads=THREADS, want_descents=True), svo.intersect(ro, rd, sh, want_descents=True))
    # an entry at coordinate 2^21 is refused and leaves the handle as it was
    before = bytes(svo.info()), svo.read_voxels()
    bad = xyz[:50].copy()
    bad[17] = (5, 1 << 21, 7)
    with pytest.raises(mv.MvrtError, match=r"entry 17 \(5, 2097152, 7\) lies outside the 2097152\^3 grid"):
        svo.edit_voxels(bad)
    assert bytes(svo.info()) == before[0]
    after = svo.read_voxels()
    assert np.array_equal(after[0], before[1][0]) and np.array_equal(after[1], before[1][1])
