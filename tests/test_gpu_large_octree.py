"""The flavour used by the HBM-bound stress configuration (BASELINE.json configs[4]): non-DAG octree, plain 32-bit
child indices with the node mask fetched from the node (voxCommon.hpp:353-356), seeded synthetic voxels generated and
built on the GPU.  Checked against the oracle at sizes it handles in seconds; bit-exact as everywhere else."""
import numpy as np
import pytest

from common import bunny_tris, hdr_bytes, position_colors, probe_camera
from fixtures import mv, O  # noqa: F401 (fixtures)
from rays import assert_hits_equal, random_rays, synthetic_reference

pytestmark = pytest.mark.gpu


def test_non_dag_non_embedded_build_and_traversal(mv, O):
    tris = bunny_tris()
    cols, emis = position_colors(tris)
    from massivevoxelraytracing_amd import scenes
    res = 256
    origin, dps = scenes.bounding_grid(tris.reshape(-1, 3), res)
    svo = mv.IntersectorOctreeGPU()
    svo.build(tris.reshape(-1, 3), cols.reshape(-1, 3), emis.reshape(-1, 3), None, origin, dps, res, flags=svo.BUILD_NO_DAG | svo.BUILD_NO_EMBEDDED_MASK)
    sc = O.build_scene_from_triangles(tris, res, cols, emis, dag=False, embed=False)
    info = svo.info()
    assert info.embeddedMask == 0 and info.numberOfNodes == len(sc.nodes) and info.numberOfVoxels == len(sc.morton)
    nodes, attrs, morton = svo.download(want_morton=True)
    got = nodes.view(O.NODE_DTYPE)
    assert np.array_equal(morton, sc.morton) and np.array_equal(attrs, sc.attrs)
    for f in ("mask", "children", "psum"):
        assert np.array_equal(got[f], sc.nodes[f]), f
    # persistent traversal, non-embedded flavour
    ro, rd = random_rays(sc, 100_000, 21)
    sh = (np.arange(len(ro)) % 4 == 0).astype(np.uint8)
    assert_hits_equal(sc.trace(ro, rd, sh, threads=8, want_descents=True), svo.intersect(ro, rd, sh, want_descents=True))
    cam = probe_camera(origin, dps, res)
    want = sc.render_primary(cam, 640, 360, show_vertex_color=True, threads=8)
    gotr = svo.render(cam, 640, 360, showVertexColor=True)
    assert np.array_equal(want["rgba"], gotr["rgba"])
    assert_hits_equal(want, gotr)
    # DAG and non-DAG octrees give the same hits
    dag = mv.IntersectorOctreeGPU()
    dag.build(tris.reshape(-1, 3), cols.reshape(-1, 3), emis.reshape(-1, 3), None, origin, dps, res)
    assert dag.info().embeddedMask == 1 and dag.info().numberOfNodes < info.numberOfNodes
    assert_hits_equal(dag.intersect(ro, rd, sh, want_descents=True), svo.intersect(ro, rd, sh, want_descents=True))


def test_path_tracer_on_non_embedded_octree(mv, O):
    tris = bunny_tris()
    cols, emis = position_colors(tris)
    sc = O.build_scene_from_triangles(tris, 128, cols, emis, dag=False, embed=False)
    rgba, hw, hh = O.decode_rgbe(hdr_bytes())
    w, h = 128, 72
    cam = probe_camera(sc.origin, sc.dps, 128, focus=9.0, lens_r=0.05)
    pt = mv.PathTracer()
    pt.setup(None)
    pt.resizeFrameBufferIfNeeded(None, w, h)
    pt.loadHDRIPixels(None, rgba, hw, hh, rgba, hw, hh)
    pt.m_intersectorOctreeGPU.upload(sc.nodes, sc.attrs, sc.origin, sc.dps, 128, sc.has_emission, embeddedMask=False)
    for _ in range(2):
        pt.step(None, cam)
    H = O.HDRI(rgba, hw, hh, rgba, hw, hh, math_mode=1)
    fb = np.zeros((w * h, 4), np.float32)
    rays = 0
    for it in range(2):
        fb, _, cnt = sc.render_pt(H, cam, w, h, it, math_mode=1, fb=fb, threads=8)
        rays += cnt["rays"]
    assert np.array_equal(pt.read_framebuffer()[: w * h], fb)
    assert pt.stats()["rays"] == rays


@pytest.mark.parametrize("res", [128, 1024])  # 1024: 10 levels, deeper than the flavour's 8-slot ring (stack entries go through the spill rows)
def test_path_tracer_on_tree_flavour(mv, O, res):
    """the GPU builder's "tree" flavour (no DAG, masks not embedded: {mask, first child} nodes + two-level bricks, hits report the voxel index
    directly -- no nVoxelsPSum walk) under the whole wavefront path tracer: frame buffer, ray and descent counters against the oracle on the
    reference-layout octree the library hands back (mvrt_svo_download), which in turn equals the oracle's own non-DAG build"""
    tris = bunny_tris()
    cols, emis = position_colors(tris)
    w, h = 150, 85
    sc = O.build_scene_from_triangles(tris, res, cols, emis, dag=False, embed=False)
    rgba, hw, hh = O.decode_rgbe(hdr_bytes())
    cam = probe_camera(sc.origin, sc.dps, res, focus=9.0, lens_r=0.05)
    pt = mv.PathTracer()
    pt.setup(None)
    pt.resizeFrameBufferIfNeeded(None, w, h)
    pt.loadHDRIPixels(None, rgba, hw, hh, rgba, hw, hh)
    svo = pt.m_intersectorOctreeGPU
    svo.build(tris.reshape(-1, 3), cols.reshape(-1, 3), emis.reshape(-1, 3), None, sc.origin, sc.dps, res, flags=svo.BUILD_NO_DAG | svo.BUILD_NO_EMBEDDED_MASK)
    nodes, attrs, _ = svo.download()
    got = nodes.view(O.NODE_DTYPE)
    for f in ("mask", "children", "psum"):
        assert np.array_equal(got[f], sc.nodes[f]), f
    assert svo.traversal_bytes() < len(sc.nodes) * 16  # 5 B per node + a 16-byte brick for every second level
    for _ in range(2):
        pt.step(None, cam)
    H = O.HDRI(rgba, hw, hh, rgba, hw, hh, math_mode=1)
    fb = np.zeros((w * h, 4), np.float32)
    tot = dict(rays=0, descents=0, shadowDescents=0, hits=0)
    for it in range(2):
        fb, _, cnt = sc.render_pt(H, cam, w, h, it, math_mode=1, fb=fb, threads=8)
        for k in tot:
            tot[k] += cnt[k]
    assert np.array_equal(pt.read_framebuffer()[: w * h], fb)
    st = pt.stats()
    for k in tot:
        assert st[k] == tot[k], k


# (the 2048^3 and 8192^3 cases: 11- and 13-level walks of the tree flavour -- deeper than its 8-slot LDS ring, so stack entries with their two mask words
# go through the HBM spill rows -- against the oracle)
@pytest.mark.parametrize("res,n,flags", [(64, 5000, 3), (256, 200_000, 1), (512, 1_000_000, 3), (128, 300_000, 0), (2048, 600_000, 3), (8192, 400_000, 3)])
def test_synthetic_octree_matches_documented_generator(mv, O, res, n, flags):
    svo = mv.IntersectorOctreeGPU()
    svo.build_synthetic(res, n, seed=1234, flags=flags)
    morton_w, attrs_w, he = synthetic_reference(O, res, n, 1234)
    dag, embed = not (flags & 1), not (flags & 2)
    nodes_w = O.build_octree(morton_w, res, dag=dag, embed=embed)
    info = svo.info()
    assert info.totalDumpedVoxels == n and info.numberOfVoxels == len(morton_w) and info.numberOfNodes == len(nodes_w)
    assert info.hasEmission == he and info.embeddedMask == int(embed)
    nodes, attrs, morton = svo.download(want_morton=True)
    got = nodes.view(O.NODE_DTYPE)
    assert np.array_equal(morton, morton_w) and np.array_equal(attrs, attrs_w)
    for f in ("mask", "children", "psum"):
        assert np.array_equal(got[f], nodes_w[f]), f
    sc = O.Scene(nodes_w, attrs_w, np.zeros(3, np.float32), np.float32(1.0 / res), res, he, embedded=embed)
    ro, rd = random_rays(sc, 50_000, res)
    assert_hits_equal(sc.trace(ro, rd, threads=8, want_descents=True), svo.intersect(ro, rd, want_descents=True))


@pytest.mark.parametrize("res,n,flags", [(2, 1, 0), (2, 64, 3), (4, 1, 1), (4, 3, 2), (8, 20_000, 0), (8, 20_000, 3), (16, 2, 0)])
def test_degenerate_octrees(mv, O, res, n, flags):
    """one-level octrees, a single voxel, a completely full grid: the edges of the traversal (root children are leaves, every
    candidate exists, almost none does), both flavours"""
    svo = mv.IntersectorOctreeGPU()
    svo.build_synthetic(res, n, seed=99, flags=flags)
    morton_w, attrs_w, he = synthetic_reference(O, res, n, 99)
    dag, embed = not (flags & 1), not (flags & 2)
    nodes_w = O.build_octree(morton_w, res, dag=dag, embed=embed)
    assert svo.info().numberOfVoxels == len(morton_w) and svo.info().numberOfNodes == len(nodes_w)
    sc = O.Scene(nodes_w, attrs_w, np.zeros(3, np.float32), np.float32(1.0 / res), res, he, embedded=embed)
    ro, rd = random_rays(sc, 30_000, 5 + res)
    # plus lattice diagonals (exact ties) through the unit cube
    k = 3000
    p = (np.random.default_rng(res).integers(0, res + 1, size=(k, 3)) / np.float32(res)).astype(np.float32)
    d = np.array([(1, 1, 1), (1, -1, 1), (-1, 1, 0.5), (0.5, 1, -1)], np.float32)[np.arange(k) % 4]
    ro = np.concatenate([ro, (p - d * np.float32(2.0)).astype(np.float32), p])
    rd = np.concatenate([rd, d, d])
    sh = (np.arange(len(ro)) % 3 == 0).astype(np.uint8)
    assert_hits_equal(sc.trace(ro, rd, sh, threads=8, want_descents=True), svo.intersect(ro, rd, sh, want_descents=True))


def test_hbm_sized_octree_properties(mv, O):
    """A non-DAG octree beyond the embedded-mask limit (> 2^24 nodes: plain 32-bit child indices, 64-bit node addressing, child masks in
    the parent's line) -- too big for the oracle, so checked through properties that do not need it: run-to-run determinism, the hit
    point lies on a face of the voxel grid perpendicular to nMajor and in front of the origin, every hit has walked all levels, shadow
    and normal rays agree on hit/miss, and a ray that starts behind its first hit and points back hits the same voxel plane."""
    res, n_vox, n_rays = 2048, 40_000_000, 400_000
    svo = mv.IntersectorOctreeGPU()
    svo.build_synthetic(res, n_vox, seed=77, flags=svo.BUILD_NO_DAG)
    info = svo.info()
    assert info.numberOfNodes >= 0xFFFFFF and info.embeddedMask == 0 and info.levels == 11
    assert 0.98 * n_vox < info.numberOfVoxels <= n_vox
    rng = np.random.default_rng(5)
    d = rng.normal(size=(n_rays, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    ro = (0.5 + 1.2 * d).astype(np.float32)
    rd = (rng.random((n_rays, 3), dtype=np.float32) - ro).astype(np.float32)
    a = svo.intersect(ro, rd, want_descents=True)
    b = svo.intersect(ro, rd, want_descents=True)
    for k in ("t", "nMajor", "vIndex", "descents"):
        assert np.array_equal(a[k], b[k]), k
    hit = a["t"] != O.MAX_FLOAT
    assert hit.sum() > 0.5 * n_rays                     # 40 M random voxels in 2048^3: almost every ray hits something
    assert (a["t"][hit] > 0).all() and (a["vIndex"][hit] < info.numberOfVoxels).all()
    assert (a["descents"][hit] >= info.levels).all()
    # hit point on a grid plane perpendicular to the reported axis (nMajor 1:x 2:y 0:z)
    p = ro[hit].astype(np.float64) + rd[hit].astype(np.float64) * a["t"][hit][:, None].astype(np.float64)
    axis = np.array([2, 0, 1])[a["nMajor"][hit]]
    c = p[np.arange(len(p)), axis] * res
    assert np.abs(c - np.round(c)).max() < 2e-3
    assert ((p > -1e-4) & (p < 1 + 1e-4)).all()
    # shadow rays report the same hit/miss
    s = svo.intersect(ro, rd, np.ones(n_rays, np.uint8))
    assert np.array_equal(s["t"] != O.MAX_FLOAT, hit)
    assert (s["vIndex"] == 0).all()
