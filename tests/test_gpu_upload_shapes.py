"""Uploaded octrees of shapes the builder never makes (tests/upload_shapes.py) on the GPU against the oracle, bit for bit: any numbering with the root
last, unreachable nodes, un-shared trees, reachable empty inner nodes and nVoxelsPSum variants, in both flavours -- traces (plain and hinted), primary
renders, path-tracer frames, the device API, read-back -- and, where the geometry and the sums are the builder's, the library's own build of the same
voxels.  Only arrays the host check accepts are uploaded (tests/test_upload_shapes_cpu.py proves the check first); a rejected upload leaves the handle's
octree in place."""
import os

import numpy as np
import pytest

import deep_scenes as D
import upload_shapes as U
from common import probe_camera
from fixtures import hdr, mv, O  # noqa: F401 (fixtures)
from rays import assert_hits_equal, compile_probe, probe_trace, random_rays
from upload_shapes import Base, bases, oracle_scene, shapes, upload, voxel_set  # noqa: F401 (bases is a fixture)

pytestmark = pytest.mark.gpu

THREADS = min(16, len(os.sched_getaffinity(0)))
MAXF = np.float32(3.402823466e38)
NO_HINT = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope="module")
def probe(mv, tmp_path_factory):
    return compile_probe(tmp_path_factory.mktemp("probe_shapes"), [])


def rays_in_voxels(base, paths, n, seed):
    """rays starting inside existing voxels (random point of the voxel, random direction) and the paths of those voxels"""
    rng = np.random.default_rng(seed)
    pick = paths[rng.integers(0, len(paths), n)]
    cell = D.decode(pick).astype(np.float64)
    p = base.origin.astype(np.float64) + (cell + 0.05 + 0.9 * rng.random((n, 3))) * float(base.dps)
    return p.astype(np.float32), rng.normal(size=(n, 3)).astype(np.float32), pick.astype(np.uint64)


SCENES = ["bunny256", "random7", "random9", "single1", "single2", "single3", "empty", "deep14"]


# ---- traces, hinted traces, read-back, the device API ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("emb", [True, False])
@pytest.mark.parametrize("scene", SCENES)
def test_uploaded_shapes_trace_like_the_oracle(mv, O, probe, bases, scene, emb):
    base = None if scene == "empty" else bases[scene]
    n_rays = 20_000 if scene in ("bunny256", "random9", "deep14") else 6000
    for name, (nodes, _) in shapes(O, base, emb, 3 + len(scene)).items():
        sc = oracle_scene(O, base, nodes, emb)
        svo = upload(mv, sc, emb)
        info = svo.info()
        assert (info.numberOfNodes, info.levels, info.embeddedMask) == (len(nodes), U.levels_of(sc.grid_res), int(emb))
        back, battrs, _ = svo.download()
        assert np.array_equal(back.view(O.NODE_DTYPE), nodes), (name, "download")
        assert np.array_equal(battrs, sc.attrs)
        if scene == "deep14":
            s = D.DeepScene(14)
            r1, r2 = s.short_rays(n_rays // 2, 5), s.long_rays(n_rays // 2, 6)
            ro, rd = np.concatenate([r1[0], r2[0]]), np.concatenate([r1[1], r2[1]])
        else:
            ro, rd = random_rays(sc, n_rays, 21)
        sh = (np.arange(len(ro)) % 3 == 0).astype(np.uint8)
        want = sc.trace(ro, rd, sh, threads=THREADS, want_descents=True)
        got = svo.intersect(ro, rd, sh, want_descents=True)
        assert_hits_equal(want, got)
        if base is not None and scene != "single1":
            assert (want["t"] != MAXF).sum() > 20, (name, "too few hits")
        if emb and base is not None:  # hints: the voxel the ray starts in, unrelated voxels, none
            paths = U.voxel_paths(nodes, sc.grid_res, emb)
            assert np.array_equal(paths, base.morton)
            hro, hrd, hint = rays_in_voxels(base, paths, n_rays // 2, 8)
            hsh = (np.arange(len(hro)) % 4 == 0).astype(np.uint8)
            hwant = sc.trace(hro, hrd, hsh, threads=THREADS, want_descents=True)
            rng = np.random.default_rng(9)
            wild = paths[rng.integers(0, len(paths), len(hro))].astype(np.uint64)
            for h in (hint, wild, np.where(rng.random(len(hro)) < 0.5, hint, NO_HINT)):
                assert_hits_equal(hwant, svo.intersect_hinted(hro, hrd, h, hsh))
            assert_hits_equal(sc.trace(ro, rd, None, threads=THREADS, want_descents=True),
                              svo.intersect_hinted(ro, rd, paths[rng.integers(0, len(paths), len(ro))].astype(np.uint64)))
        if U.levels_of(sc.grid_res) <= 16 and base is not None:  # the device API (both stack modes)
            view = svo.device_view()
            for mode in (0, 1):
                p = probe_trace(mv, probe, view, ro, rd, sh, mode)
                for k in ("t", "nMajor", "vIndex", "descents"):
                    assert np.array_equal(p[k], got[k]), (name, mode, k)


@pytest.mark.parametrize("emb", [True, False])
@pytest.mark.parametrize("scene", ["bunny256", "random7", "random9", "single2"])
def test_shapes_that_keep_the_builder_answers_equal_the_library_build(mv, O, bases, scene, emb):
    """independent of the oracle: the library's own build of the same voxel list gives the same t, nMajor, vIndex and descents"""
    base = bases[scene]
    built = mv.IntersectorOctreeGPU()
    built.build_voxels(D.decode(base.morton), base.attrs, origin=base.origin, dps=base.dps, gridRes=base.res, flags=0)
    sc0 = oracle_scene(O, base, O.build_octree(base.morton, base.res, embed=emb), emb)
    ro, rd = random_rays(sc0, 20_000, 31)
    sh = (np.arange(len(ro)) % 5 == 0).astype(np.uint8)
    want = built.intersect(ro, rd, sh, want_descents=True)
    for name, (nodes, keeps) in shapes(O, base, emb, 40).items():
        if not keeps:
            continue
        got = upload(mv, oracle_scene(O, base, nodes, emb), emb).intersect(ro, rd, sh, want_descents=True)
        for k in ("t", "nMajor", "vIndex", "descents"):
            assert np.array_equal(got[k], want[k]), (name, k)


# ---- renders -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("emb", [True, False])
@pytest.mark.parametrize("scene", ["bunny256", "random7", "random9", "single3", "empty"])
def test_uploaded_shapes_render_primary_like_the_oracle(mv, O, bases, scene, emb):
    base = None if scene == "empty" else bases[scene]
    for name, (nodes, _) in shapes(O, base, emb, 50).items():
        sc = oracle_scene(O, base, nodes, emb)
        cam = probe_camera(sc.origin, sc.dps, sc.grid_res)
        got = upload(mv, sc, emb).render(cam, 96, 56, showVertexColor=True)
        want = sc.render_primary(cam, 96, 56, show_vertex_color=True, threads=THREADS)
        assert_hits_equal(want, got)
        assert np.array_equal(want["rgba"], got["rgba"]), name


@pytest.mark.parametrize("emb", [True, False])
@pytest.mark.parametrize("scene", ["bunny256", "random9"])
def test_uploaded_shapes_path_trace_like_the_oracle(mv, O, bases, hdr, scene, emb):
    rgba, hw, hh = hdr
    H = O.HDRI(rgba, hw, hh, rgba, hw, hh, math_mode=1)
    w, h = 48, 32
    base = bases[scene]
    for name, (nodes, _) in shapes(O, base, emb, 60).items():
        sc = oracle_scene(O, base, nodes, emb)
        cam = probe_camera(sc.origin, sc.dps, sc.grid_res, focus=9.0, lens_r=0.05, offset=(1.5, 1.0, 1.5) if scene != "bunny256" else (6, 4, 6))
        fb, sl, cnt = sc.render_pt(H, cam, w, h, 0, math_mode=1, want_samples=True, threads=THREADS)
        assert cnt["hits"] > 100, name
        for hints in (True, False):
            pt = mv.PathTracer()
            pt.setup(None)
            pt.resizeFrameBufferIfNeeded(None, w, h)
            pt.loadHDRIPixels(None, rgba, hw, hh, rgba, hw, hh)
            upload(mv, sc, emb, pt.m_intersectorOctreeGPU)
            pt.set_origin_hints(hints)
            pt.step(None, cam)
            assert np.array_equal(pt.sample_radiance()[: w * h * 16], sl), (name, hints)
            assert np.array_equal(pt.read_framebuffer()[: w * h], fb), (name, hints)
            st = pt.stats()
            for k in ("rays", "shadowRays", "descents", "shadowDescents", "hits"):
                assert st[k] == cnt[k], (name, hints, k, st[k], cnt[k])
            del pt


# ---- a rejected upload leaves the octree in place ----------------------------------------------------------------------------------------------
def test_rejected_upload_keeps_the_octree(mv, O, bases):
    base = bases["random7"]
    sc = oracle_scene(O, base, O.build_octree(base.morton, base.res), True)
    svo = upload(mv, sc, True)
    ro, rd = random_rays(sc, 20_000, 41)
    before = svo.intersect(ro, rd, want_descents=True)
    info0 = svo.info()
    rng = np.random.default_rng(42)
    t = (sc.nodes, len(base.morton), base.res, True)
    for name in ("coarse_voxel", "grid_halved", "self_loop", "child_out_of_range", "psum_reaches_count", "wrong_embedded_byte"):
        nodes, nv, res, emb = U.MUTATIONS[name](t, rng)[:4]
        with pytest.raises(mv.MvrtError, match="rule"):
            svo.upload(nodes, base.attrs[:max(nv, 1)] if nv else np.zeros((0, 8), np.uint8), base.origin, base.dps, res, base.he, embeddedMask=emb)
        after = svo.intersect(ro, rd, want_descents=True)
        for k in ("t", "nMajor", "vIndex", "descents"):
            assert np.array_equal(after[k], before[k]), (name, k)
        info = svo.info()
        assert (info.numberOfNodes, info.numberOfVoxels, info.gridRes) == (info0.numberOfNodes, info0.numberOfVoxels, info0.gridRes)
    assert np.array_equal(before["t"], sc.trace(ro, rd, threads=THREADS)["t"])
