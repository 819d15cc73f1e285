"""Cone-limited rays on the MI355X: mvrt_trace_batch_cone and a user kernel on intersectCone / DeviceLod of include/mvrt/device.hpp (tests/hip/cone_probe.hip, both
stack modes) against the scalar model of tests/lod_expected.py, bit for bit in t, nMajor, level, cellCode and descents on every ray -- uploaded and GPU-built
octrees, embedded and plain, the bunny at 2^3 .. 64^3 and the hand-made sets (a lone corner voxel; two voxels of one coarse cell with rays passing between them;
two subtrees of equal shape and different colours, whose nodes the DAG shares).  The model is validated against the oracle first (tests/test_cone_walk_cpu.py
holds the same on the CPU).

Independent of the model: with coneB = 0 and coneA = dps * 2^(levels - D) the walk stops at depth D, and t and nMajor equal the oracle's Scene.trace on the
octree built from the codes >> 3 (levels - D), on every ray from outside, for every D.  The attribute pyramid equals mvrt_svo_coarse_voxels of the same handle and
the numpy model of tests/coarsen_expected.py per level, the index and attribute of every cone hit come from it, and whatever changes the voxels drops it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lod_expected as L
import surface_expected as S
from common import probe_camera
from fixtures import mv, O  # noqa: F401 (fixtures)
from voxel_mesh_app import read_ppm, run_app, write_obj

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
f32 = np.float32


@pytest.fixture(scope="module")
def probe(mv, tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("cone_probe")), "cone_probe.so")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "hip", "cone_probe.hip"), "-o", so], timeout=300)
    lib = C.CDLL(so)
    lib.probe_cone.restype = C.c_int
    lib.probe_cone.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64] + [C.c_void_p] * 15 + [C.c_int]
    return lib


def probe_cone(mv, probe, view, lod, ro, rd, cone_a, cone_b, mode):
    n = len(ro)
    dev = [mv.DeviceArray.from_host(np.ascontiguousarray(a)) for a in (ro[:, 0], ro[:, 1], ro[:, 2], rd[:, 0], rd[:, 1], rd[:, 2], cone_a, cone_b)]
    out = [mv.DeviceArray(n, d) for d in L.TYPES] + [mv.DeviceArray(n, np.uint32), mv.DeviceArray((n, 8), np.uint8)]
    rc = probe.probe_cone(C.byref(view), None if lod is None else C.byref(lod), n, *[a.ptr for a in dev], *[a.ptr for a in out], mode)
    assert rc == 0, rc
    got = dict(zip(L.OUTPUTS + ("index", "attribs"), (a.to_host() for a in out)))
    if lod is None:
        del got["index"], got["attribs"]
    return got


def upload(mv, sc, embedded):
    svo = mv.IntersectorOctreeGPU()
    svo.upload(sc.nodes, sc.attrs, sc.origin, sc.dps, sc.grid_res, sc.has_emission, embeddedMask=embedded)
    return svo


def built(mv, s, flags=0):
    svo = mv.IntersectorOctreeGPU()
    svo.build_voxels(s.xyz, s.attribs, origin=s.sc.origin, dps=s.sc.dps, gridRes=s.res, flags=flags)
    return svo


def same(got, want, keys, what):
    for k in keys:
        a, b = (np.ascontiguousarray(x[k]).view(np.uint8).reshape(len(x[k]), -1) for x in (got, want))
        eq = a.shape == b.shape and (a == b).all(1)
        assert np.all(eq), "%s: %s differs on %d of %d rays, first at %d" % (what, k, (~eq).sum(), eq.size, np.argmax(~eq))


def no_pyramid(mv, svo):
    assert svo.lod_bytes() == 0
    with pytest.raises(mv.MvrtError, match="mvrt_svo_lod_view: no attribute pyramid"):
        svo.lod_view()


@pytest.mark.parametrize("source", ["uploaded", "built"])
@pytest.mark.parametrize("embedded", [True, False], ids=["embedded", "plain"])
@pytest.mark.parametrize("scene", L.SCENES)
def test_cone_rays_equal_the_model(mv, O, probe, scene, embedded, source):
    s = L.scene(O, scene, embedded)
    s.validate()
    svo = upload(mv, s.sc, embedded) if source == "uploaded" else built(mv, s, 0 if embedded else 2)
    view = svo.device_view()
    assert view.flavour == (0 if embedded else 1) and view.levels == s.levels
    assert np.array_equal(np.array(view.lower[:], f32), s.lower) and np.array_equal(np.array(view.upper[:], f32), s.upper)
    lod = None
    if source == "built":
        svo.lod_prepare()
        lod = svo.lod_view()
        assert lod.structBytes == C.sizeof(mv.DeviceLod) and lod.levels == s.levels
    got = [svo.intersect_cone(s.ro, s.rd, s.cone_a, s.cone_b, want_attribs=lod is not None)]
    got += [probe_cone(mv, probe, view, lod, s.ro, s.rd, s.cone_a, s.cone_b, mode) for mode in (0, 1)]
    for i, g in enumerate(got):
        same(g, s.on, L.OUTPUTS, "%s, %s" % (scene, ("mvrt_trace_batch_cone", "probe, own stack", "probe, caller's stack")[i]))
    if lod is not None:  # the index and the attribute of every hit, from the numpy model of the coarsening
        index, attribs = s.attrib_of(s.on)
        for g in got:
            assert np.array_equal(g["index"], index) and np.array_equal(g["attribs"], attribs)
        assert (attribs[s.on["level"] == 0] == 0).all()
    # the identities of the rule against mvrt_trace_batch, the streaming kernel
    unlimited = svo.intersect(s.ro, s.rd, None, want_descents=True)
    same(unlimited, s.off, ("t", "nMajor", "descents"), scene + ", mvrt_trace_batch")
    cone = got[0]
    with np.errstate(invalid="ignore"):
        no_cone = ~((s.cone_a > 0) | (s.cone_b > 0))  # zero, negative and NaN
    assert no_cone.sum() >= len(s.ro) // 8
    same({k: cone[k][no_cone] for k in cone}, {k: unlimited[k][no_cone] for k in unlimited}, ("t", "nMajor", "descents"), scene + ", no cone")
    assert (cone["descents"] <= unlimited["descents"]).all()
    hit, hit_cone = unlimited["t"] != L.MAXF, cone["t"] != L.MAXF
    assert hit_cone[hit].all()
    if s.levels > 1:
        inf = np.isinf(s.cone_a) & (s.cone_a > 0) & (s.cone_b == 0) & s.outside & hit_cone
        assert inf.sum() >= 10 and (cone["level"][inf] == 1).all()  # +inf stops at level 1
        assert len(set(cone["level"][hit_cone].tolist())) == s.levels  # every inner level and the voxels
    if scene == "between":
        assert (hit_cone & ~hit).sum() >= 10  # a ray between the two voxels of one coarse cell: the cone hits, the unlimited ray misses
    if scene == "twins" and lod is not None:  # one node, two colours
        at2 = got[0]["attribs"][cone["level"] == 2]
        assert {tuple(a[:3]) for a in at2.tolist()} == {(200, 40, 10), (10, 60, 220)}


@pytest.mark.parametrize("scene", [n for n in L.SCENES if n != "bunny2"])
def test_fixed_depth_equals_the_coarsened_octree(mv, O, scene):
    """independent of the model: coneB = 0, coneA = dps * 2^(levels - D) against the oracle on the octree of D levels, every ray from outside"""
    s = L.scene(O, scene)
    svo = upload(mv, s.sc, True)
    ro, rd = s.ro[s.outside], s.rd[s.outside]
    full = svo.intersect(ro, rd, None, want_descents=True)
    for D in range(1, s.levels):
        sc, cells = s.coarse_scene(O, D)
        want = sc.trace(ro, rd, None, threads=8)
        got = svo.intersect_cone(ro, rd, f32(s.sc.dps) * f32(2.0 ** (s.levels - D)), f32(0))
        same(got, want, ("t", "nMajor"), "%s, depth %d" % (scene, D))
        hit = want["t"] != L.MAXF
        assert hit.sum() >= 100 and (got["level"][hit] == D).all() and (got["level"][~hit] == 0).all()
        assert np.array_equal(got["cellCode"][hit], cells[want["vIndex"][hit]]) and (got["cellCode"][~hit] == 0).all()
        assert (got["descents"] <= full["descents"]).all()


@pytest.mark.parametrize("flags", [0, 2])
@pytest.mark.parametrize("scene", L.SCENES)
def test_pyramid_equals_the_coarse_listing(mv, O, scene, flags):
    s = L.scene(O, scene)
    svo = built(mv, s, flags)
    no_pyramid(mv, svo)
    nbytes = svo.lod_prepare()
    v = svo.lod_view()
    total = 0
    for lv in range(1, s.levels):
        got, want = svo.lod_level(lv), s.level(lv)
        listed = svo.coarse_voxels(s.levels - lv, 1)
        assert np.array_equal(got["code"], S.morton(listed["xyz"].astype(np.int64))) and np.array_equal(got["attribs"], listed["attribs"])
        assert np.array_equal(got["count"], listed["count"])
        for k in ("code", "attribs", "count"):
            assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (lv, k)
        assert got["count"].sum() == len(s.codes) and v.count[lv] == len(want["code"])
        total += len(want["code"]) * 20
    assert nbytes == total == svo.lod_bytes() and (total > 0) == (s.levels > 1)  # a one-level octree: an empty pyramid, and the call succeeds
    assert v.count[s.levels] == len(s.codes) and v.codes[0] == 0 and v.count[0] == 0 and v.cellVoxels[s.levels] == 0
    assert all(v.codes[k] == 0 and v.count[k] == 0 for k in range(s.levels + 1, 17))
    assert svo.lod_prepare() == total  # again: replaced, not added
    svo.lod_release()
    no_pyramid(mv, svo)


def test_pyramid_goes_with_the_voxels_it_describes(mv, O):
    import gc
    s = L.scene(O, "bunny32")
    gc.collect()
    base = mv.allocation_state()[:2]
    svo = built(mv, s)

    def prepared():
        before = mv.allocation_state()[1]
        assert svo.lod_prepare() > 0 and svo.lod_bytes() > 0
        assert mv.allocation_state()[1] - before == svo.lod_bytes()  # the pyramid's memory is the owner's: counted, and nothing else stays

    prepared()
    svo.edit_voxels(s.xyz[:3], np.full((3, 8), 7, np.uint8))  # attributes only: written in place
    assert svo.info().numberOfVoxels == len(s.codes)
    no_pyramid(mv, svo)
    prepared()
    assert svo.lod_level(s.levels - 1)["attribs"].shape[1] == 8
    svo.edit_voxels(s.xyz[:3], None, np.zeros(3, np.uint8))  # structural: three voxels removed
    assert svo.info().numberOfVoxels == len(s.codes) - 3
    no_pyramid(mv, svo)
    prepared()
    svo.build_voxels(s.xyz, s.attribs, origin=s.sc.origin, dps=s.sc.dps, gridRes=s.res)
    no_pyramid(mv, svo)
    # the voxel-set operators.  A combine that only recolours writes the attributes in place, outside the edit's route
    other_attribs = (255 - s.attribs).astype(np.uint8)
    other_attribs[:, [3, 7]] = 255
    other = mv.IntersectorOctreeGPU()
    other.build_voxels(s.xyz, other_attribs, origin=s.sc.origin, dps=s.sc.dps, gridRes=s.res)
    prepared()
    before = svo.lod_level(s.levels - 1)
    assert svo.combine(svo, mv.COMBINE_UNION) == (0, 0, 0) and svo.lod_bytes() > 0  # nothing changes: the handle is not touched
    assert svo.combine(other, mv.COMBINE_UNION, flags=mv.COMBINE_ATTRIB_B) == (0, 0, 0)
    assert np.array_equal(svo.read_voxels()[1], other_attribs)
    no_pyramid(mv, svo)
    prepared()
    after, want = svo.lod_level(s.levels - 1), L.CE.coarse(s.xyz, other_attribs, 1)
    assert np.array_equal(after["attribs"], want["attribs"]) and not np.array_equal(after["attribs"], before["attribs"])
    first = built(mv, s)
    assert svo.transfer_attributes(first)[0] > 0  # attributes only, through the edit's route
    assert np.array_equal(svo.read_voxels()[1], s.attribs)
    no_pyramid(mv, svo)
    first.cleanUp()
    other.cleanUp()
    prepared()
    assert svo.dilate(mv.MORPH_FACES, 1) > 0  # structural
    no_pyramid(mv, svo)
    prepared()
    assert svo.erode(mv.MORPH_FACES, 1) > 0
    no_pyramid(mv, svo)
    prepared()
    svo.coarsen(1)  # in place
    assert svo.info().gridRes == s.res // 2
    no_pyramid(mv, svo)
    prepared()
    svo.rebuild(2)
    no_pyramid(mv, svo)
    prepared()
    svo.upload(s.sc.nodes, s.sc.attrs, s.sc.origin, s.sc.dps, s.sc.grid_res, 1)
    no_pyramid(mv, svo)
    svo.cleanUp()
    assert mv.allocation_state()[:2] == base


def test_refusals_and_the_empty_batch(mv, O):
    s = L.scene(O, "bunny8")
    lib = mv.lib()
    up, bt = upload(mv, s.sc, True), built(mv, s)
    out = up.intersect_cone(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0), np.zeros(0))
    assert all(len(out[k]) == 0 for k in L.OUTPUTS)
    assert lib.mvrt_trace_batch_cone(up._h, 0, *([None] * 6), 1, 1, 1, *([None] * 6), None) == 0  # no launch: the pointers are never read
    # NULL required arrays: before the handle is looked at
    one = mv.DeviceArray(4, np.float32)
    rays = [one.ptr] * 6
    for args, word in (((None, one.ptr, one.ptr), "coneADev and coneBDev are required"), ((one.ptr, None, one.ptr), "coneADev and coneBDev are required"),
                       ((one.ptr, one.ptr, None), "t output is required")):
        assert lib.mvrt_trace_batch_cone(None, 1, *rays, *args, *([None] * 6), None) != 0
        assert word in lib.mvrt_last_error().decode()
    assert lib.mvrt_trace_batch_cone(None, 1, *([None] * 6), one.ptr, one.ptr, one.ptr, *([None] * 6), None) != 0
    assert "null ray array" in lib.mvrt_last_error().decode()
    assert lib.mvrt_trace_batch_cone(None, 1, *rays, one.ptr, one.ptr, one.ptr, *([None] * 6), None) != 0
    assert "no octree" in lib.mvrt_last_error().decode()
    empty = mv.IntersectorOctreeGPU()
    z = np.zeros((4, 3), f32)
    with pytest.raises(mv.MvrtError, match="mvrt_trace_batch_cone: no octree"):
        empty.intersect_cone(z, z + 1, 0, 0)
    with pytest.raises(mv.MvrtError, match="mvrt_svo_lod_prepare: no octree"):
        empty.lod_prepare()
    with pytest.raises(mv.MvrtError, match="mvrt_svo_lod_prepare: an uploaded octree keeps no Morton codes"):
        up.lod_prepare()
    # index and attribute need the pyramid, by name; everything else does not, uploads included
    for svo in (up, bt):
        with pytest.raises(mv.MvrtError, match="mvrt_trace_batch_cone: indexDev needs the attribute pyramid"):
            svo.intersect_cone(z, z + 1, 0, 0, want_attribs=True)
        four = [mv.DeviceArray(4, np.float32) for _ in range(9)]
        at = mv.DeviceArray((4, 8), np.uint8)
        with pytest.raises(mv.MvrtError, match="mvrt_trace_batch_cone: attribDev needs the attribute pyramid"):
            svo.intersect_cone_device(4, *four, attrib=at)
        with pytest.raises(mv.MvrtError, match="mvrt_render_primary_lod: showVertexColor needs the attribute pyramid"):
            svo.render_lod(probe_camera(s.sc.origin, s.sc.dps, s.res), 8, 8, 1.0, showVertexColor=True)
        assert len(svo.render_lod(probe_camera(s.sc.origin, s.sc.dps, s.res), 8, 8, 1.0)["t"]) == 64
    tree = mv.IntersectorOctreeGPU()
    tree.build_voxels(s.xyz, s.attribs, origin=s.sc.origin, dps=s.sc.dps, gridRes=s.res, flags=mv.IntersectorOctreeGPU.BUILD_NO_DAG | mv.IntersectorOctreeGPU.BUILD_NO_EMBEDDED_MASK)
    assert tree.info().flavour == 2
    with pytest.raises(mv.MvrtError, match="mvrt_trace_batch_cone: tree-flavour"):
        tree.intersect_cone(z, z + 1, 0, 0)
    with pytest.raises(mv.MvrtError, match="mvrt_svo_lod_prepare: tree-flavour"):
        tree.lod_prepare()
    with pytest.raises(mv.MvrtError, match="mvrt_render_primary_lod: tree-flavour"):
        tree.render_lod(probe_camera(s.sc.origin, s.sc.dps, s.res), 8, 8, 1.0)


W, H = 64, 48


@pytest.mark.parametrize("embedded", [True, False], ids=["embedded", "plain"])
def test_render_lod(mv, O, embedded):
    s = L.scene(O, "bunny64", embedded)
    svo = built(mv, s, 0 if embedded else 2)
    svo.lod_prepare()
    ext = float(f32(s.sc.dps) * f32(s.res))
    cam = probe_camera(s.sc.origin, s.sc.dps, s.res, offset=(1.2 * ext, 0.8 * ext, 1.15 * ext))
    for colour in (False, True):  # lodScale = 0: mvrt_render_primary in every output
        want, got = svo.render(cam, W, H, showVertexColor=colour), svo.render_lod(cam, W, H, 0.0, showVertexColor=colour)
        same(got, want, ("rgba", "t", "nMajor", "descents"), "lodScale 0")
        hit = want["t"] != L.MAXF
        assert hit.sum() >= 500 and (got["level"][hit] == s.levels).all() and (got["level"][~hit] == 0).all()
    # lodScale = 1: the model on the oracle's rays through the pixel centres
    rays = [O.camera_shoot(cam, x, y, 0.5, 0.5, W, H) for y in range(H) for x in range(W)]
    ro, rd = np.array([r[0] for r in rays], f32), np.array([r[1] for r in rays], f32)
    cone_b = f32(1.0) * ((f32(2.0) * cam[12]) / f32(H))
    model = L.trace(s.tree, ro, rd, f32(0), cone_b)
    levels = np.bincount(model["level"], minlength=s.levels + 1)
    print("render_lod: pixels per level", levels.tolist())
    assert (levels[1:] >= 50).sum() >= 2  # the image mixes levels
    got = svo.render_lod(cam, W, H, 1.0, showVertexColor=True)
    same(got, model, ("t", "nMajor", "level", "descents"), "lodScale 1")
    rgba = s.attrib_of(model)[1][:, :4].copy()
    rgba[model["level"] == 0] = (0, 0, 0, 255)
    assert np.array_equal(got["rgba"], rgba)
    normals = svo.render_lod(cam, W, H, 1.0)  # without showVertexColor: the hit normal, as mvrt_render_primary paints it
    same(normals, model, ("t", "nMajor", "level"), "lodScale 1, normals")
    hit = model["level"] != 0
    n = np.array([O.get_hit_n(m, d) for m, d in zip(model["nMajor"][hit], rd[hit])], f32)
    want = np.full((len(n), 4), 255, np.uint8)
    want[:, :3] = (f32(255) * ((n + f32(1)) * f32(0.5)) + f32(0.5)).astype(np.uint8)
    assert np.array_equal(normals["rgba"][hit], want) and (normals["rgba"][~hit] == (0, 0, 0, 255)).all()
    assert (got["descents"] <= svo.render(cam, W, H)["descents"]).all()


def test_device_render_lod_equals_render_lod(mv, tmp_path):
    """apps/device_render --lod: an application kernel on intersectCone and DeviceLod paints the image of mvrt_render_primary_lod"""
    from common import bunny_tris, position_colors
    from massivevoxelraytracing_amd import build as b, scenes
    b.build_apps(verbose=False)
    exe = os.path.join(ROOT, "apps", "device_render")
    tris = bunny_tris()
    v = tris.reshape(-1, 3)
    cols = position_colors(tris)[0].reshape(-1, 3)
    obj = str(tmp_path / "bunny.obj")
    write_obj(obj, v, cols)
    res, w, h = 128, 160, 90
    origin, dps = scenes.bounding_grid(v, res)
    svo = mv.IntersectorOctreeGPU()
    svo.build(v, cols, np.zeros_like(v), None, origin, dps, res)
    svo.lod_prepare()
    ext = float(f32(dps) * f32(res))
    cam = probe_camera(origin, dps, res, offset=(1.2 * ext, 0.8 * ext, 1.15 * ext))
    r = subprocess.run([exe, obj, str(tmp_path / "no.ppm"), "--lod", "1", "--sun", "0", "1", "0"], capture_output=True, text=True)
    assert r.returncode == 2 and "--lod and --sun" in r.stderr and not os.path.exists(str(tmp_path / "no.ppm"))  # refused before anything is built
    for colour in (False, True):
        out, prefix = str(tmp_path / ("lod%d.ppm" % colour)), str(tmp_path / ("lod%d" % colour))
        run_app(exe, [obj, out, "--size", str(w), str(h), "--res", str(res), "--lod", "2", "--camera"] + ["%.9g" % c for c in cam] + ["--dump", prefix] +
                (["--vertex-color"] if colour else []))
        want = svo.render_lod(cam, w, h, 2.0, showVertexColor=colour)
        hit = want["level"] != 0
        assert hit.sum() > 1000 and (want["level"][hit] < 7).sum() > 100  # rays stopped above the voxels
        assert np.array_equal(read_ppm(out, w, h), want["rgba"][:, :3])
        assert np.array_equal(np.fromfile(prefix + ".t.f32", np.float32), want["t"])
        assert np.array_equal(np.fromfile(prefix + ".nmajor.i32", np.int32), want["nMajor"])
