"""The HIP kernels against the COMPILED reference directly (oracle/_ref/libmvrt_ref_walk.so; never the reference tree): the voxelizer and the builder
on the triangles where voxelizers go wrong -- vertices on lattice points, triangles in lattice planes, equal vertices, slivers, clipped and sub-voxel
triangles -- and the traversal on the ray set of tests/test_reference_pins_cpu.py.  The other GPU tests compare with the oracle, which is a restatement
of the reference written together with the kernels; these do not go through it.  Where oracle/_ref is absent the kernels must reproduce the stored
SHA-256 of the reference's answer (tests/reference_pins.py::check).  All comparisons are exact.

The renderer's sampling code is compared with oracle/_ref/libmvrt_ref_render.so (the host branch of renderCommon.hpp / pmjSampler.hpp) wherever no
transcendental is involved: the PMJ table on the device, the device header's camera, the primary cast and the first-hit buffers of one path-tracing step,
whose rays are the work of kPtGenerate (PMJ dimensions 0 and 1, their scrambles, the thin lens).

Colours and emission are compared with the oracle, as everywhere: the reference's barycentric code (closestBarycentricCoordinateOnTriangle) sits in
voxKernel.cu, which no host compiler here builds."""
import numpy as np
import pytest

import reference_pins as R
from common import hdr_bytes
from fixtures import mv, O  # noqa: F401 (fixtures)
from rays import compile_probe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def walk(O):
    return R.load_walk(O, tree_decides=False)


def build_and_compare(mv, O, walk, key, tris, origin, dps, res, flags):
    cols, emis = R.vertex_attributes(len(tris), 41)
    svo = mv.IntersectorOctreeGPU()
    svo.build(tris.reshape(-1, 3), cols.reshape(-1, 3), emis.reshape(-1, 3), None, origin, dps, res, flags=flags)
    info = svo.info()
    nodes, attrs, morton = svo.download(want_morton=True)
    nodes = nodes.view(O.NODE_DTYPE)
    assert info.numberOfVoxels == len(morton) and info.numberOfNodes == len(nodes)
    R.check(key, [np.array([info.totalDumpedVoxels], np.uint64), morton] + R.node_fields(nodes), walk,
            lambda w: R.reference_build(w, tris, origin, dps, res, flags))
    # attributes: the oracle's, merged like the reference's `unique` kernel merges them
    m, a = O.voxelize(tris, origin, dps, res, cols, emis, six_separating=not (flags & R.CONSERVATIVE))
    m, a, he = O.merge_voxels(m, a)
    assert np.array_equal(m, morton) and np.array_equal(a, attrs) and info.hasEmission == he


CLASS_CASES = R.class_build_cases()


@pytest.mark.parametrize("case", CLASS_CASES, ids=[c[0] for c in CLASS_CASES])
def test_triangle_class_builds(mv, O, walk, case):
    """dumped count, the sorted unique voxel list and the embedded DAG nodes of each class (plus one ordinary triangle), 32^3 and 4^3, six-separating
    and conservative"""
    build_and_compare(mv, O, walk, *case)


@pytest.mark.parametrize("flags", [0, R.CONSERVATIVE])
@pytest.mark.parametrize("res", [32, 4])
def test_equal_vertices_alone_touch_no_voxel(mv, res, flags):
    """the reference finds no voxel for a triangle with two equal vertices (tests/test_reference_pins_cpu.py asserts the counts are 0); a mesh of nothing
    else is refused by name"""
    origin, dps = R.class_grid(res)
    tris = R.triangle_classes(res)["two_equal"]
    svo = mv.IntersectorOctreeGPU()
    with pytest.raises(mv.MvrtError, match="touch no voxel"):
        svo.build(tris.reshape(-1, 3), None, None, None, origin, dps, res, flags=flags)


MIXED_CASES = R.mixed_build_cases()


@pytest.mark.parametrize("case", MIXED_CASES, ids=[c[0] for c in MIXED_CASES])
def test_all_classes_between_bunny_triangles(mv, O, walk, case):
    """every class dealt between 3000 bunny triangles at 256^3, footprints on both sides of the whole-wave threshold: the lane-own and the whole-wave path
    of kVoxelize run in the same waves"""
    tris, origin, dps, res = case[1:5]
    v = tris.reshape(-1, 3, 3)
    lo = np.clip(np.floor((v.min(1) - origin) / dps), 0, res - 1)
    hi = np.clip(np.floor((v.max(1) - origin) / dps), 0, res - 1)
    ext = np.sort(hi - lo + 1, axis=1)
    assert (ext[:, 0] * ext[:, 1] > 2048).sum() > 20 and (ext[:, 1] * ext[:, 2] <= 2048).sum() > 3000  # whatever the major axis: some big, most small
    build_and_compare(mv, O, walk, *case)


@pytest.mark.parametrize("scene", R.FAR_SCENES)
def test_trace_batch(mv, O, walk, scene):
    """one mvrt_trace_batch of the CPU pin's whole ray set -- ties, origins on voxel corners / edges / faces, secondary-style origins, direction
    components of +-0, denormals, +-inf and NaN, a third shadow rays -- against the reference's traversal: t by its bits, nMajor and vIndex on all rays.
    A second call traces the CPU pin's far-origin rays (origins up to 2^23 extents away; the fast loop of traceStream had seen 4 extents at most)."""
    rs = R.ray_scene(O, scene)
    ro, rd, sh = R.rays_of(O, scene)
    svo = mv.IntersectorOctreeGPU()
    svo.upload(rs.nodes, rs.sc.attrs, rs.sc.origin, rs.sc.dps, rs.sc.grid_res, rs.sc.has_emission)
    info = svo.info()
    assert np.array_equal(np.array(info.lower[:], np.float32), rs.lower) and np.array_equal(np.array(info.upper[:], np.float32), rs.upper)
    got = svo.intersect(ro, rd, sh)
    R.check("trace/" + scene, [got["t"], got["nMajor"], got["vIndex"]], walk,
            lambda w: [x for x in w.trace(rs.nodes, rs.lower, rs.upper, ro, rd, sh).values()])
    fro, frd, fsh, _ = R.far_rays_of(O, scene, R.N_FAR_PIN)
    far = svo.intersect(fro, frd, fsh)
    assert ((far["t"] != R.MAXF) & (far["t"] > 2.0 ** 20 * rs.dps * rs.sc.grid_res)).sum() > 1000
    R.check("trace_far/" + scene, [far["t"], far["nMajor"], far["vIndex"]], walk,
            lambda w: [x for x in w.trace(rs.nodes, rs.lower, rs.upper, fro, frd, fsh).values()])


# ---- the renderer's sampling code against oracle/_ref/libmvrt_ref_render.so, not through the oracle ------------------------------------------------
@pytest.fixture(scope="module")
def render(O):
    return R.load_render(O, tree_decides=False)


@pytest.fixture(scope="module")
def pair(render, walk):
    """(render library, walk library), or None where oracle/_ref is absent: then the stored digests of the same compositions stand in"""
    return None if render is None or walk is None else (render, walk)


def test_pmj_table_on_the_device(mv, render):
    """the table as read back from the device equals the table of the reference's PMJSampler::setup( false, ... ), float by float"""
    pt = mv.PathTracer()
    pt.setup(None)
    R.check("render/pmj_table", [pt.pmj_table()], render, lambda r: [r.pmj_table()])


def test_device_camera(mv, render, tmp_path_factory):
    """mvrt::CameraPinhole::shoot / shootThinLens of include/mvrt/device.hpp, run on the device by tests/hip/device_api_probe.hip: corner pixels, offsets and
    lens samples at 0 and at the float below 1, odd and non-square sizes, an orthonormal and a skewed basis -- 2736 rays per camera and entry point"""
    probe = compile_probe(tmp_path_factory.mktemp("camera_probe"), [])
    px, fl = R.camera_rays()
    dpx, dfl = mv.DeviceArray.from_host(px), mv.DeviceArray.from_host(fl)
    for name, cam in R.cameras().items():
        for thin in (0, 1):
            ro, rd = mv.DeviceArray((len(px), 3), np.float32), mv.DeviceArray((len(px), 3), np.float32)
            assert probe.probe_camera(cam.ctypes.data, len(px), dpx.ptr, dfl.ptr, thin, ro.ptr, rd.ptr) == 0
            R.check("render/camera/%s/%d" % (name, thin), [ro.to_host(), rd.to_host()], render, lambda r: list(r.camera_shoot(cam, px, fl, bool(thin))))


@pytest.fixture(scope="module")
def frame(mv, O):
    sc = R.frame_scene(O)
    svo = mv.IntersectorOctreeGPU()
    svo.upload(sc.nodes, sc.attrs, sc.origin, sc.dps, sc.grid_res, sc.has_emission)
    info = svo.info()
    lower, upper = sc.bounds()
    assert np.array_equal(np.array(info.lower[:], np.float32), lower) and np.array_equal(np.array(info.upper[:], np.float32), upper)
    return sc, svo


@pytest.mark.parametrize("size", R.PRIMARY_SIZES, ids=["%dx%d" % s for s in R.PRIMARY_SIZES])
@pytest.mark.parametrize("cam", ["outside", "inside"])
def test_primary_cast(mv, O, pair, frame, cam, size):
    """render( ..., want_hits=True ) of the bunny at 64^3 against the reference composed here: shoot from the render library through every pixel centre, then
    octreeTraverse_EfficientParametric from the walk library.  t by its bits, nMajor and vIndex on every pixel, misses included."""
    sc, svo = frame
    W, H = size
    c = R.frame_cameras(sc)[cam]
    got = svo.render(c, W, H, want_hits=True)
    hit = got["t"] != R.MAXF
    assert 0.1 < hit.mean() and (cam == "inside" or hit.mean() < 0.9) and len(np.unique(got["nMajor"][hit])) == 3
    R.check("render/primary/%s/%dx%d" % (cam, W, H), [got["t"], got["nMajor"], got["vIndex"]], pair, lambda p: R.reference_primary(p, sc, c, W, H))


@pytest.mark.parametrize("cam", ["outside", "inside"])
def test_first_hit_buffers(mv, O, pair, frame, cam):
    """the normal / depth buffer of one 16-spp step at 64x40, lensR 0.05, against rays built from the compiled reference alone: sample2d (dimensions 0 and 1,
    stream = Murmur of the pixel, spp 0 .. 15) and shootThinLens from the render library, then the walk library's traversal.  This checks kPtGenerate's
    dimensions, scrambles and thin lens against the reference directly.  Depth is a derived quantity: the buffer stores no single t but the sum of the 16
    samples' first-hit t (and of their axis normals), added in ascending sample order in float32 -- tests/aov_expected.py restates that sum, once, for
    the oracle's and the reference's rays alike; with the rays equal to the reference's, the sums are equal by their bits."""
    sc, _ = frame
    W, H = R.FIRST_HIT_SIZE
    c = R.frame_cameras(sc)[cam]
    assert c[13] == np.float32(0.05)
    rgba, hw, hh = O.decode_rgbe(hdr_bytes())
    pt = mv.PathTracer()
    pt.setup(None)
    pt.set_aovs(True)
    pt.resizeFrameBufferIfNeeded(None, W, H)
    pt.loadHDRIPixels(None, rgba, hw, hh, rgba, hw, hh)
    pt.m_intersectorOctreeGPU.upload(sc.nodes, sc.attrs, sc.origin, sc.dps, sc.grid_res, sc.has_emission)
    pt.step(None, c)
    nd = pt.read_aov(pt.AOV_NORMAL_DEPTH)[: W * H]
    hits = pt.read_aov(pt.AOV_ALBEDO)[: W * H, 3]
    assert ((hits > 0) & (hits < 16)).sum() >= 30 and (hits == 16).sum() >= 100  # partly covered pixels: the order and the set of the samples matter
    R.check("render/first_hit/" + cam, [nd], pair, lambda p: R.reference_first_hit(p, O, sc, c))
