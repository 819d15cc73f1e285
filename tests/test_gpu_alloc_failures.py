"""Every device allocation of a call is made to fail in turn (mvrt_test_fail_allocation), on small scenes.  After each failure the handle holds a
whole octree / HDRI map / frame or none, nothing in between (include/mvrt.h, "What a failed call leaves behind"): the state is read with host queries
first, an empty handle is never launched on, and an intact one still gives the results recorded before the sweep bit for bit.  The same call without
the hook then succeeds and matches the oracle.  mvrt_test_allocation_state counts the buffers: a failed call leaks nothing."""
import gc

import numpy as np
import pytest

from alloc_sweep import mv  # noqa: F401 (the fixture)
from common import bunny_tris, hdr_bytes, position_colors, probe_camera
from fixtures import O  # noqa: F401 (fixtures)
from rays import splitmix64

pytestmark = pytest.mark.gpu

RES, W, H, NRAYS = 256, 64, 36, 20_000
INFO_FIELDS = ("numberOfNodes", "numberOfVoxels", "dps", "emissionScale", "hasEmission", "embeddedMask", "gridRes", "levels", "totalDumpedVoxels", "flavour")


@pytest.fixture(scope="module")
def bunny(O):
    tris = bunny_tris()
    cols, emis = position_colors(tris)
    return O.build_scene_from_triangles(tris, RES, cols, emis)


@pytest.fixture(autouse=True)
def no_buffer_outlives_its_handles(mv):
    gc.collect()
    before = mv.allocation_state()[0]
    yield
    mv.set_test_fail_allocation(0)
    gc.collect()
    assert mv.allocation_state()[0] == before  # every handle of the test is destroyed: nothing is left


def live(mv):
    return mv.allocation_state()[0]


def info_of(svo):
    i = svo.info()
    return tuple(getattr(i, f) for f in INFO_FIELDS) + (tuple(i.lower), tuple(i.upper))


def mixed_rays(sc, n, seed):
    """from outside and inside the volume, axis-parallel and zero-component directions among them (tests/rays.py), a third of them shadow rays"""
    rng = np.random.default_rng(seed)
    lo, hi = sc.bounds()
    ro = ((lo + hi) / 2 + (rng.random((n, 3)) - 0.5) * (hi - lo).max() * 2.5).astype(np.float32)
    rd = ((lo + rng.random((n, 3)) * (hi - lo)).astype(np.float32) - ro).astype(np.float32)
    k = n // 10
    rd[:k, 0] = 0.0
    rd[k:2 * k, 1] = 0.0
    rd[2 * k:3 * k, 2] = 0.0
    rd[3 * k:3 * k + 50] = np.array([0, 0, -1], np.float32)
    ro[4 * k:5 * k] = (lo + rng.random((k, 3)) * (hi - lo)).astype(np.float32)
    return ro, rd, (np.arange(n) % 3 == 0).astype(np.uint8)


def same_hits(a, b):
    return all(np.array_equal(a[f], b[f]) for f in ("t", "nMajor", "vIndex", "descents"))


def assert_oracle_hits(want, got):
    assert np.array_equal(want["t"], got["t"]) and np.array_equal(want["descents"], got["descents"])
    hit = want["t"] != np.float32(3.402823466e38)
    assert np.array_equal(want["nMajor"][hit], got["nMajor"][hit]) and np.array_equal(want["vIndex"][hit], got["vIndex"][hit])
    assert (got["nMajor"][~hit] == -1).all()


def assert_octree(O, svo, sc, rays, want_hits):
    """the handle holds the oracle's octree `sc`: nodes in the reference layout, attributes, and the hits of the mixed rays"""
    i = svo.info()
    assert (i.numberOfNodes, i.numberOfVoxels, i.hasEmission) == (len(sc.nodes), len(sc.attrs), sc.has_emission)
    gn, ga, _ = svo.download()
    got = gn.view(O.NODE_DTYPE)
    for f in ("mask", "children", "psum"):
        assert np.array_equal(got[f], sc.nodes[f]), f
    assert np.array_equal(ga, sc.attrs)
    assert_oracle_hits(want_hits, svo.intersect(*rays, want_descents=True))


def assert_refuses_empty(mv, svo, pt=None, cam=None):
    """host queries only: an empty handle says so and every entry point that reads an octree returns an error (no launch)"""
    i = svo.info()
    assert i.numberOfNodes == 0 and i.numberOfVoxels == 0
    assert svo.traversal_bytes() == 0 and not svo.m_nodeBuffer and not svo.m_vAttributeBuffer
    d = mv.DeviceArray(4, np.float32)
    for call in (lambda: svo.intersect_device(1, d, d, d, d, d, d, None, d, d, d), svo.device_view, svo.read_voxels, svo.download,
                 lambda: svo.edit_voxels(np.zeros((1, 3), np.uint32))):
        with pytest.raises(mv.MvrtError, match="no octree"):
            call()
    if pt is not None:
        with pytest.raises(mv.MvrtError, match="no scene"):
            pt.step(None, cam)


def count_allocations(mv, call):
    t0 = mv.allocation_state()[2]
    call()
    n = mv.allocation_state()[2] - t0
    assert n >= 1
    return n


def fail_nth(mv, n, call):
    """arm, call, and see the call fail on exactly that allocation; returns the change of the number of live buffers"""
    before = live(mv)
    mv.set_test_fail_allocation(n)
    with pytest.raises(mv.MvrtError, match="mvrt_test_fail_allocation"):
        call()
    assert mv.lib().mvrt_test_fail_allocation(0) == 0  # (it has disarmed itself; this is for a test that fails above)
    return live(mv) - before


def path_tracer(mv, scale0=True):
    pt = mv.PathTracer()
    pt.setup(None)
    if scale0:
        pt.set_hdri_scale(0.0)
    return pt


# ---- calls that release the old octree first: every failure leaves the handle empty -------------------------------------------------------------------
def sweep_always_empty(mv, O, call, sc, check=None):
    """`call( svo )` replaces the octree of a path tracer's intersector by `sc` (the oracle's)"""
    pt = path_tracer(mv)
    pt.resizeFrameBufferIfNeeded(None, W, H)
    svo = pt.m_intersectorOctreeGPU
    svo.set_emission_scale(3.25)
    cam = probe_camera(sc.origin, sc.dps, sc.grid_res, focus=9.0, lens_r=0.05)
    rays = mixed_rays(sc, NRAYS, 11)
    rays = (rays[0], rays[1], rays[2])
    want = sc.trace(*rays, threads=8, want_descents=True)
    base = live(mv)
    n = count_allocations(mv, lambda: call(svo))
    held = live(mv) - base  # buffers of one resident octree
    assert held >= 3
    whole = info_of(svo)
    for k in range(1, n + 1):
        assert info_of(svo) == whole  # the octree of the last successful call is replaced
        before = live(mv)  # (with the handle's traversal workspace, which stays)
        assert fail_nth(mv, k, lambda: call(svo)) == -held, k
        assert_refuses_empty(mv, svo, pt, cam)
        assert svo.info().emissionScale == 3.25
        call(svo)
        assert info_of(svo) == whole and live(mv) == before
        (check or assert_octree)(O, svo, sc, rays, want)
    print("allocations failed in turn:", n, "-- buffers of the octree:", held)
    pt.step(None, cam)  # ... and the path tracer renders it
    assert pt.read_framebuffer()[: W * H, 3].min() == 16
    return n


@pytest.mark.parametrize("embedded", [True, False])
def test_upload(mv, O, bunny, embedded):
    sc = bunny if embedded else O.Scene(O.build_octree(bunny.morton, RES, dag=True, embed=False), bunny.attrs, bunny.origin, bunny.dps, RES, bunny.has_emission, embedded=False)
    n = sweep_always_empty(mv, O, lambda svo: svo.upload(sc.nodes, sc.attrs, sc.origin, sc.dps, RES, sc.has_emission, embeddedMask=embedded), sc)
    assert n >= 5  # the staged nodes, nodes, masks, attributes and a fifth array of either flavour


@pytest.mark.parametrize("flags", [0, 3])  # default; MVRT_BUILD_NO_DAG | MVRT_BUILD_NO_EMBEDDED_MASK (the tree flavour)
def test_build_ex(mv, O, bunny, flags):
    tris = bunny_tris()
    cols, emis = position_colors(tris)
    sc = bunny if flags == 0 else O.Scene(O.build_octree(bunny.morton, RES, dag=False, embed=False), bunny.attrs, bunny.origin, bunny.dps, RES, bunny.has_emission, embedded=False)
    v, c, e = tris.reshape(-1, 3), cols.reshape(-1, 3), emis.reshape(-1, 3)
    sweep_always_empty(mv, O, lambda svo: svo.build(v, c, e, None, sc.origin, sc.dps, RES, flags=flags), sc)


def synthetic_voxels(O, res, n, seed):
    """numpy restatement of the documented generator (include/mvrt.h) + the oracle's merge, as tests/test_gpu_large_octree.py"""
    with np.errstate(over="ignore"):
        h = splitmix64(np.uint64(seed) + np.arange(n, dtype=np.uint64))
        c = splitmix64(h)
    m = np.uint64(res - 1)
    xyz = np.stack([h & m, (h >> np.uint64(21)) & m, (h >> np.uint64(42)) & m], -1).astype(np.uint32)
    rgb = (c & np.uint64(0xFFFFFF)) | np.uint64(0x404040)
    em = np.where((c >> np.uint64(56)) == 0, rgb, np.uint64(0))
    attrs = np.full((n, 8), 255, np.uint8)
    for k in range(3):
        attrs[:, k] = ((rgb >> np.uint64(8 * k)) & np.uint64(255)).astype(np.uint8)
        attrs[:, 4 + k] = ((em >> np.uint64(8 * k)) & np.uint64(255)).astype(np.uint8)
    return O.merge_voxels(O.morton_encode_batch(xyz), attrs)


def test_build_synthetic(mv, O):
    res, nv, seed = 64, 5000, 3
    morton, attrs, he = synthetic_voxels(O, res, nv, seed)
    sc = O.Scene(O.build_octree(morton, res), attrs, np.zeros(3, np.float32), np.float32(1.0 / res), res, he)
    sweep_always_empty(mv, O, lambda svo: svo.build_synthetic(res, nv, seed), sc)


# ---- voxel lists: the old octree stays until the new arrays exist -----------------------------------------------------------------------------------------
def decode(m):
    m = np.asarray(m, np.uint64)
    out = np.zeros((len(m), 3), np.uint32)
    for axis in range(3):
        for b in range(21):
            out[:, axis] |= (((m >> np.uint64(3 * b + axis)) & np.uint64(1)) << np.uint64(b)).astype(np.uint32)
    return out


def sweep_old_or_empty(mv, O, restore, call, old, new, want_attrs_only=False):
    """`restore( svo )` puts the octree `old` into the handle, `call( svo )` turns it into `new` (both the oracle's).  A failure leaves `old` or nothing."""
    svo = mv.IntersectorOctreeGPU()
    rays = mixed_rays(old, NRAYS, 12)
    want_old, want_new = (s.trace(*rays, threads=8, want_descents=True) for s in (old, new))
    base = live(mv)
    restore(svo)
    held = live(mv) - base
    assert_octree(O, svo, old, rays, want_old)
    before = (info_of(svo), svo.intersect(*rays, want_descents=True), svo.download(want_morton=True))  # (the first trace allocates the handle's workspace)
    base = live(mv) - held
    n = count_allocations(mv, lambda: call(svo))
    assert_octree(O, svo, new, rays, want_new)
    ends = []
    for k in range(1, n + 1):
        restore(svo)
        assert info_of(svo) == before[0] and live(mv) == base + held
        delta = fail_nth(mv, k, lambda: call(svo))
        if svo.info().numberOfNodes == 0:
            ends.append("empty")
            assert delta == -held, k
            assert_refuses_empty(mv, svo)
        else:
            ends.append("old")
            assert delta == 0, k
            assert info_of(svo) == before[0]
            assert same_hits(svo.intersect(*rays, want_descents=True), before[1])
            assert all(np.array_equal(x, y) for x, y in zip(svo.download(want_morton=True), before[2]))
            assert live(mv) == base + held
        if svo.info().numberOfNodes == 0:
            restore(svo)
        call(svo)
        assert_octree(O, svo, new, rays, want_new)
    print("allocations failed in turn:", n, "-- old octree kept by the first", ends.count("old"), "-- buffers of the octree:", held)
    assert ends == sorted(ends, reverse=True)  # the old octree up to one point of the call, none from there on
    assert ends[0] == "old" and (want_attrs_only or ends[-1] == "empty")
    if want_attrs_only:
        assert set(ends) == {"old"}
    return n


def voxel_scene(O, bunny, morton, attrs):
    m, a, he = O.merge_voxels(morton, attrs)
    sc = O.Scene(O.build_octree(m, RES), a, bunny.origin, bunny.dps, RES, he)
    sc.morton = m
    return sc


def test_build_voxels(mv, O, bunny):
    rng = np.random.default_rng(5)
    keep = rng.random(len(bunny.morton)) < 0.7
    new = voxel_scene(O, bunny, bunny.morton[keep], bunny.attrs[keep])
    xyz_old, xyz_new = decode(bunny.morton), decode(new.morton)
    sweep_old_or_empty(mv, O, lambda svo: svo.build_voxels(xyz_old, bunny.attrs, origin=bunny.origin, dps=bunny.dps, gridRes=RES),
                       lambda svo: svo.build_voxels(xyz_new, new.attrs, origin=bunny.origin, dps=bunny.dps, gridRes=RES), bunny, new)


def test_edit_voxels_structural(mv, O, bunny):
    rng = np.random.default_rng(6)
    gone = rng.random(len(bunny.morton)) < 0.1
    fresh = rng.integers(0, RES, size=(3000, 3), dtype=np.uint32)
    fresh_attrs = rng.integers(0, 256, size=(3000, 8), dtype=np.uint8)
    fresh_attrs[:, 3] = fresh_attrs[:, 7] = 255
    fm, first = np.unique(O.morton_encode_batch(fresh)[::-1], return_index=True)  # the last entry per voxel wins
    fa = fresh_attrs[::-1][first]
    d = {int(k): bunny.attrs[i] for i, k in enumerate(bunny.morton) if not gone[i]}
    d.update({int(k): fa[i] for i, k in enumerate(fm)})
    ks = np.array(sorted(d), np.uint64)
    new = voxel_scene(O, bunny, ks, np.array([d[int(k)] for k in ks], np.uint8))
    xyz_old = decode(bunny.morton)
    xyz = np.concatenate([xyz_old[gone], fresh])
    attrs = np.concatenate([bunny.attrs[gone], fresh_attrs])
    ops = np.concatenate([np.zeros(int(gone.sum()), np.uint8), np.ones(len(fresh), np.uint8)])
    sweep_old_or_empty(mv, O, lambda svo: svo.build_voxels(xyz_old, bunny.attrs, origin=bunny.origin, dps=bunny.dps, gridRes=RES),
                       lambda svo: svo.edit_voxels(xyz, attrs, ops), bunny, new)


def test_edit_voxels_attributes_only(mv, O, bunny):
    rng = np.random.default_rng(7)
    pick = rng.choice(len(bunny.morton), 5000, replace=False)
    attrs = bunny.attrs.copy()
    attrs[pick, :3] = rng.integers(0, 256, size=(len(pick), 3), dtype=np.uint8)
    new = voxel_scene(O, bunny, bunny.morton, attrs)
    xyz_old = decode(bunny.morton)
    sweep_old_or_empty(mv, O, lambda svo: svo.build_voxels(xyz_old, bunny.attrs, origin=bunny.origin, dps=bunny.dps, gridRes=RES),
                       lambda svo: svo.edit_voxels(xyz_old[pick], attrs[pick]), bunny, new, want_attrs_only=True)


# ---- path tracer: HDRI maps and frames ------------------------------------------------------------------------------------------------------------------------
def frame(pt, cam):
    pt.clearFrameBuffer(None)
    pt.step(None, cam)
    return pt.read_framebuffer()[: W * H]


def scene_pt(mv, bunny, scale0):
    pt = path_tracer(mv, scale0)
    pt.m_intersectorOctreeGPU.upload(bunny.nodes, bunny.attrs, bunny.origin, bunny.dps, RES, bunny.has_emission)
    pt.resizeFrameBufferIfNeeded(None, W, H)
    return pt, probe_camera(bunny.origin, bunny.dps, RES, focus=9.0, lens_r=0.05)


def test_first_hdri_load(mv, O, bunny):
    rgba, hw, hh = O.decode_rgbe(hdr_bytes())
    pt, cam = scene_pt(mv, bunny, scale0=True)
    without = frame(pt, cam)
    hd = O.HDRI(rgba, hw, hh, rgba, hw, hh, math_mode=1)
    want, _, _ = bunny.render_pt(hd, cam, W, H, 0, math_mode=1, threads=8)
    n = count_allocations(mv, lambda: pt.loadHDRIPixels(None, rgba, hw, hh, rgba, hw, hh))
    assert n >= 10  # pixels, scratch, seven tables, the primary map
    for k in range(1, n + 1):
        fresh, _ = scene_pt(mv, bunny, scale0=True)
        assert fail_nth(mv, k, lambda: fresh.loadHDRIPixels(None, rgba, hw, hh, rgba, hw, hh)) == 0, k
        for which in range(7):
            with pytest.raises(mv.MvrtError, match="no such HDRI table"):
                fresh.hdri_sat(which, hw, hh)
        assert np.array_equal(frame(fresh, cam), without)  # no map, as before
        fresh.set_hdri_scale(1.75)
        with pytest.raises(mv.MvrtError, match="HDRI enabled"):
            fresh.step(None, cam)
        fresh.loadHDRIPixels(None, rgba, hw, hh, rgba, hw, hh)
        assert np.array_equal(frame(fresh, cam), want)


def test_hdri_load_over_a_map(mv, O, bunny):
    rgba, hw, hh = O.decode_rgbe(hdr_bytes())
    other = np.ascontiguousarray(rgba.reshape(hh, hw, 4)[::-1] * np.float32(0.5)).reshape(-1, 4)  # another map: upside down, half as bright
    ow, oh = hw, hh
    pt, cam = scene_pt(mv, bunny, scale0=False)
    pt.loadHDRIPixels(None, rgba, hw, hh, rgba, hw, hh)
    before = frame(pt, cam)
    tables = [pt.hdri_sat(i, hw, hh) for i in range(7)]
    want_before, _, _ = bunny.render_pt(O.HDRI(rgba, hw, hh, rgba, hw, hh, math_mode=1), cam, W, H, 0, math_mode=1, threads=8)
    want_other, _, _ = bunny.render_pt(O.HDRI(other, ow, oh, other, ow, oh, math_mode=1), cam, W, H, 0, math_mode=1, threads=8)
    assert np.array_equal(before, want_before) and not np.array_equal(want_before, want_other)
    n = count_allocations(mv, lambda: pt.loadHDRIPixels(None, other, ow, oh, other, ow, oh))
    for k in range(1, n + 1):
        pt.loadHDRIPixels(None, rgba, hw, hh, rgba, hw, hh)
        assert fail_nth(mv, k, lambda: pt.loadHDRIPixels(None, other, ow, oh, other, ow, oh)) == 0, k
        assert all(np.array_equal(pt.hdri_sat(i, hw, hh), tables[i]) for i in range(7))
        assert np.array_equal(frame(pt, cam), before)  # the map loaded before, fully in place
        pt.loadHDRIPixels(None, other, ow, oh, other, ow, oh)
        assert np.array_equal(frame(pt, cam), want_other)


@pytest.fixture(scope="module")
def bunny_frame(O, bunny):
    """the probe camera and the oracle's first step of the bunny at W x H without an HDRI map (path_tracer's scale 0)"""
    rgba, hw, hh = O.decode_rgbe(hdr_bytes())
    hd = O.HDRI(rgba, hw, hh, rgba, hw, hh, math_mode=1)
    hd.set_scale(0.0)
    cam = probe_camera(bunny.origin, bunny.dps, RES, focus=9.0, lens_r=0.05)
    want, _, _ = bunny.render_pt(hd, cam, W, H, 0, math_mode=1, threads=8)
    return cam, want


def assert_no_frame(mv, pt, cam):
    for call in (lambda: pt.step(None, cam), pt.resolve, pt.read_framebuffer, pt.clearFrameBuffer):
        with pytest.raises(mv.MvrtError, match="no frame buffer"):
            call()


@pytest.mark.parametrize("moments", [False, True])
@pytest.mark.parametrize("aovs", [False, True])
def test_resize_framebuffer(mv, bunny, bunny_frame, aovs, moments):
    cam, want = bunny_frame

    def fresh():
        pt = path_tracer(mv)
        pt.m_intersectorOctreeGPU.upload(bunny.nodes, bunny.attrs, bunny.origin, bunny.dps, RES, bunny.has_emission)
        pt.set_aovs(aovs)
        pt.set_moments(moments)
        return pt

    ref = fresh()
    base = live(mv)
    ref.resizeFrameBufferIfNeeded(None, 48, 27)
    held = live(mv) - base - 1  # buffers of one frame (- 1: the counters of a path tracer, allocated once with its first frame and kept)
    assert held >= 5
    n = count_allocations(mv, lambda: ref.resizeFrameBufferIfNeeded(None, W, H))  # (a frame of another size over the first one)
    assert np.array_equal(frame(ref, cam), want)
    want_aovs = [ref.read_aov(i) for i in (0, 1)] if aovs else []
    want_moments = ref.read_moments() if moments else None
    pt = fresh()
    pt.resizeFrameBufferIfNeeded(None, 48, 27)
    for k in range(1, n + 1):
        pt.resizeFrameBufferIfNeeded(None, 48, 27)
        assert fail_nth(mv, k, lambda: pt.resizeFrameBufferIfNeeded(None, W, H)) == -held, k
        assert_no_frame(mv, pt, cam)
        if aovs:
            assert not pt.aov_dev(0) and not pt.aov_dev(1)
        if moments:
            assert not pt.moments_dev()
        pt.resizeFrameBufferIfNeeded(None, W, H)
        assert np.array_equal(frame(pt, cam), want)
        assert all(np.array_equal(pt.read_aov(i), w) for i, w in zip((0, 1), want_aovs))
        if moments:
            assert np.array_equal(pt.read_moments(), want_moments)


# The calls that reallocate the path state under a live frame.  own: how many of the call's first allocations are the option's own accumulation buffers, beside
# a frame that is not touched yet; buffers: what the option adds to read, once it is on
REALLOCATING_CALLS = {
    "set_aovs": (lambda pt: pt.set_aovs(True), 2, lambda pt: [pt.read_aov(0), pt.read_aov(1)]),
    "set_moments": (lambda pt: pt.set_moments(True), 1, lambda pt: [pt.read_moments()]),
    "set_batch_steps": (lambda pt: pt.set_batch_steps(2), 0, lambda pt: []),
    "set_pipeline_depth": (lambda pt: pt.set_pipeline_depth(2), 0, lambda pt: []),
}


def assert_option_off(mv, pt, name):
    if name == "set_aovs":
        assert not pt.aov_dev(0) and not pt.aov_dev(1)
        with pytest.raises(mv.MvrtError, match="feature buffers are off"):
            pt.read_aov(0)
    if name == "set_moments":
        assert not pt.moments_dev()
        with pytest.raises(mv.MvrtError, match="moments are off"):
            pt.read_moments()


@pytest.mark.parametrize("name", list(REALLOCATING_CALLS))
def test_reallocation_under_a_live_frame(mv, bunny, bunny_frame, name):
    """Every allocation of the call fails in turn on a cleared frame.  What is left is (a) the frame as it was, the option off -- only while the option's own
    accumulation buffers are being allocated -- or (b) no frame at all, from which a resize recovers."""
    call, own, buffers = REALLOCATING_CALLS[name]
    cam, want = bunny_frame

    def fresh():
        pt = path_tracer(mv)
        pt.m_intersectorOctreeGPU.upload(bunny.nodes, bunny.attrs, bunny.origin, bunny.dps, RES, bunny.has_emission)
        base = live(mv)
        pt.resizeFrameBufferIfNeeded(None, W, H)
        held = live(mv) - base - 1  # buffers of the frame (- 1: the counters of a path tracer, kept)
        pt.clearFrameBuffer(None)
        assert pt.getSteps() == 0
        return pt, held

    twin, held = fresh()
    assert held >= 5
    n = count_allocations(mv, lambda: call(twin))
    assert n > own
    assert np.array_equal(frame(twin, cam), want)
    want_buffers = buffers(twin)
    ends = []
    for k in range(1, n + 1):
        pt, _ = fresh()
        delta = fail_nth(mv, k, lambda: call(pt))
        if delta == 0:  # (a)
            ends.append("a")
            assert k <= own, k
            assert_option_off(mv, pt, name)
            assert np.array_equal(frame(pt, cam), want)
            continue
        ends.append("b")
        assert delta == -held, k
        assert_no_frame(mv, pt, cam)
        pt.resizeFrameBufferIfNeeded(None, W, H)
        assert np.array_equal(frame(pt, cam), want)
        pt.clearFrameBuffer(None)
        call(pt)  # ... and with the option on
        assert np.array_equal(frame(pt, cam), want)
        assert all(np.array_equal(x, y) for x, y in zip(buffers(pt), want_buffers))
    print(name, "-- allocations failed in turn:", n, "-- ends:", "".join(ends), "-- buffers of the frame:", held)
