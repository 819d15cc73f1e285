"""The level of detail from the voxels themselves on the GPU (mvrt_svo_coarse_voxels / mvrt_svo_coarsen) against the numpy model of tests/coarsen_expected.py:
the listing's xyz, attribs, count and n bit for bit, the sizing call, and the coarsened octree byte for byte the one build_voxels builds from the model's list --
on the smallest inputs that can break each mechanism: aligned runs of 8, 64 and 512, one cell that holds the whole list across the wave seam, the workgroup seam
and more than two workgroups, random sets with runs on both sides of every seam, runs that start in a workgroup's last lane or end in its first, the 21-bit edge
(a shift of 60 bits), every minCount regime, sums beyond 32 bits, every flavour of source, edits, fills, a rebuilt upload -- and the contract of the two calls."""
import ctypes as C
import os

import numpy as np
import pytest

import coarsen_expected as X
import surface_expected as S
from common import GOLDEN, bunny_tris, probe_camera
from fixtures import mv  # noqa: F401 (fixtures)
from voxel_sets import DPS, LOWER, assert_same_octree, filled, full, shell

pytestmark = pytest.mark.gpu

B = 1024  # entries per workgroup of the reduce kernel (CB, csrc/kernels_coarsen.hip): 256 threads, four consecutive entries each; a wave covers 256 entries


def build(mv, xyz, res, flags=0, attribs=None, origin=LOWER, dps=DPS):
    svo = mv.IntersectorOctreeGPU()
    attribs = None if attribs is None else np.ascontiguousarray(attribs, np.uint8)
    svo.build_voxels(np.ascontiguousarray(xyz, np.uint32), attribs, origin=origin, dps=dps, gridRes=res, flags=flags)
    return svo


INFO_FIELDS = ("numberOfNodes", "numberOfVoxels", "lower", "upper", "dps", "emissionScale", "hasEmission", "embeddedMask", "gridRes", "levels", "flavour", "reserved")


def info_of(svo):
    i = svo.info()
    out = {f: getattr(i, f) for f in INFO_FIELDS}
    for f in ("lower", "upper"):
        out[f] = np.array(out[f][:], np.float32).tobytes()
    out["dps"] = np.float32(out["dps"]).tobytes()
    return out


def assert_listing(svo, want, k, min_count=1):
    got = svo.coarse_voxels(k, min_count)
    n = len(want["xyz"])
    print("k", k, "minCount", min_count, "cells", len(got["xyz"]), "model", n)
    assert svo.coarse_voxels_device(k, min_count) == n  # the sizing call
    for f, dtype in (("xyz", np.uint32), ("attribs", np.uint8), ("count", np.uint32)):
        assert got[f].dtype == dtype and got[f].shape == want[f].shape and np.array_equal(got[f], want[f]), f


def assert_coarsened(mv, src, want, n_fine, res, k, min_count=1, flags=0, dst=None):
    """src.coarsen into dst (None: a fresh handle) leaves the octree build_voxels builds from the model's list"""
    before = info_of(src)
    dst = mv.IntersectorOctreeGPU() if dst is None else dst
    scale = dst.info().emissionScale  # the destination's own: the call does not touch it
    assert src.coarsen(k, min_count, flags, dst) is dst
    twin = build(mv, want["xyz"], res >> k, flags, want["attribs"], origin=np.frombuffer(before["lower"], np.float32),
                 dps=np.float32(np.frombuffer(before["dps"], np.float32)[0] * np.float32(2 ** k)))
    twin.set_emission_scale(scale)
    assert_same_octree(dst, twin, skip=("totalDumpedVoxels",))  # the coarsening hands adoptSortedOnGrid the source's voxel count (csrc/api.hip), asserted below
    assert dst.info().totalDumpedVoxels == n_fine and info_of(dst)["upper"] == before["upper"]  # the same box, bit for bit
    return dst


def check(mv, xyz, attribs, res, k, min_count=1, flags=0, src_flags=0):
    want = X.coarse(xyz, attribs, k, min_count)
    if len(xyz) <= 6000:
        assert X.same(want, X.coarse_loop(xyz, attribs, k, min_count))
    src = build(mv, xyz, res, src_flags, attribs)
    held = src.download(want_morton=True)
    assert_listing(src, want, k, min_count)
    if len(want["xyz"]):
        assert_coarsened(mv, src, want, len(xyz), res, k, min_count, flags)
    assert all(np.array_equal(a, b) for a, b in zip(src.download(want_morton=True), held))  # the source is only read
    return src, want


def random_attribs(rng, n):
    return rng.integers(0, 256, size=(n, 8), dtype=np.uint8)


def cells_with_counts(rng, k, counts):
    """counts[j] random voxels of the coarse cell with Morton code j, in Morton order: entry i of the sorted list lies where the cumulated counts put it"""
    codes = [(np.uint64(j) << np.uint64(3 * k)) | np.sort(rng.choice(8 ** k, size=c, replace=False)).astype(np.uint64) for j, c in enumerate(counts) if c]
    return S.decode(np.concatenate(codes))


# ---- tiny grids and aligned runs -----------------------------------------------------------------------------------------------------------------------------------
def test_smallest_grid(mv):
    check(mv, [(3, 1, 2)], [(9, 8, 7, 1, 6, 5, 4, 2)], 4, 1)
    _, want = check(mv, full(4), random_attribs(np.random.default_rng(1), 64), 4, 1)  # 8 runs of 8
    assert want["count"].tolist() == [8] * 8


@pytest.mark.parametrize("k", [1, 2, 3])
def test_full_grid_has_aligned_runs(mv, k):
    _, want = check(mv, full(16), random_attribs(np.random.default_rng(k), 4096), 16, k)
    assert (want["count"] == 8 ** k).all() and len(want["count"]) == 4096 >> (3 * k)


# ---- one cell that holds the whole list: the wave seam, the workgroup seam, atomics from more than two workgroups ---------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, B - 1, B, B + 1, 2 * B + 1, 5 * B + 3])
def test_one_cell_holds_the_whole_list(mv, n):
    rng = np.random.default_rng(n)
    xyz = cells_with_counts(rng, 5, [0, 0, 0, 0, 0, n])  # cell 5 of the 2^3 grid over 64^3
    _, want = check(mv, xyz, random_attribs(rng, n), 64, 5)
    assert want["xyz"].tolist() == [[1, 0, 1]] and want["count"].tolist() == [n]


# ---- random sets: short runs, long runs and singletons on both sides of every seam --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cloud():
    rng = np.random.default_rng(20)
    xyz = np.argwhere(rng.random((64, 64, 64)) < 0.076)
    return xyz, random_attribs(rng, len(xyz))


@pytest.mark.parametrize("min_count", [1, 3])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_random_sets(mv, cloud, k, min_count):
    xyz, attribs = cloud
    assert 19000 < len(xyz) < 21000
    _, want = check(mv, xyz, attribs, 64, k, min_count, flags=(k % 4))
    assert len(want["xyz"]) > 0


def test_dense_blob_has_long_and_short_runs(mv):
    rng = np.random.default_rng(21)
    xyz = np.unique(np.concatenate([np.argwhere(rng.random((32, 32, 32)) < 0.8), np.argwhere(rng.random((64, 64, 64)) < 0.004)]), axis=0)
    for k in (3, 4):
        _, want = check(mv, xyz, random_attribs(rng, len(xyz)), 64, k)
        assert want["count"].max() > 300 and (k == 4 or want["count"].min() == 1)


def test_a_long_run_starts_in_the_last_lane_of_a_workgroup(mv):
    rng = np.random.default_rng(22)
    xyz = cells_with_counts(rng, 4, [B - 1, 2 * B - 48, 5, 0, 1, 700])  # the second cell's run: entries B - 1 .. 3 B - 50, through the whole second workgroup
    _, want = check(mv, xyz, random_attribs(rng, len(xyz)), 64, 4)
    assert want["count"].tolist() == [B - 1, 2 * B - 48, 5, 1, 700]


def test_a_long_run_ends_in_the_first_lane_of_a_workgroup(mv):
    rng = np.random.default_rng(23)
    xyz = cells_with_counts(rng, 4, [300, B - 299, 3, 1, 0, 2 * B - 5, 1])  # the second cell's run: entries 300 .. B; the sixth ends with the third workgroup, the last entry stands alone in a fourth
    _, want = check(mv, xyz, random_attribs(rng, len(xyz)), 64, 4)
    assert want["count"].tolist() == [300, B - 299, 3, 1, 2 * B - 5, 1] and 300 + B - 299 == B + 1 and 300 + B - 299 + 4 + 2 * B - 5 == 3 * B


# ---- the 21-bit edge ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 20])
def test_corners_of_the_largest_grid(mv, k):
    res = 1 << 21
    top = res - 1
    xyz = [(0, 0, 0), (1, 0, 0), (top, top, top), (top - 1, top, top), (top, top - 1, top - 1), (5, 4, 3)]
    src, want = check(mv, xyz, random_attribs(np.random.default_rng(k), len(xyz)), res, k)
    assert src.info().levels == 21 and want["xyz"].max() == (top >> k)
    if k == 20:  # a shift of 60 bits; the coarse grid is 2^3
        assert want["xyz"].tolist() == [[0, 0, 0], [1, 1, 1]] and want["count"].tolist() == [3, 3]


# ---- minCount --------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_count", [1, 2, 8])
def test_min_count_on_cells_of_every_count(mv, min_count):
    rng = np.random.default_rng(30)
    xyz = cells_with_counts(rng, 1, [1, 2, 3, 4, 5, 6, 7, 8, 0, 8, 1, 7])
    _, want = check(mv, xyz, random_attribs(rng, len(xyz)), 8, 1, min_count)
    assert sorted(want["count"].tolist()) == sorted(c for c in [1, 2, 3, 4, 5, 6, 7, 8, 8, 1, 7] if c >= min_count)


def test_a_min_count_that_keeps_nothing(mv):
    rng = np.random.default_rng(31)
    xyz = cells_with_counts(rng, 1, [1, 2, 3, 0, 3])
    src, want = check(mv, xyz, None, 8, 1, 4)
    assert len(want["xyz"]) == 0 and src.coarse_voxels_device(1, 4) == 0  # a success with 0 cells
    got = src.coarse_voxels(1, 4)
    assert got["xyz"].shape == (0, 3) and got["count"].shape == (0,)
    dst = build(mv, full(4), 4)
    for d in (dst, src):  # another handle, and in place: refused, the destination unchanged
        held, info = d.download(want_morton=True), bytes(d.info())
        with pytest.raises(mv.MvrtError, match="would leave no voxel"):
            src.coarsen(1, 4, 0, d)
        assert bytes(d.info()) == info and all(np.array_equal(a, b) for a, b in zip(d.download(want_morton=True), held))


def test_a_lone_emitter_dims_to_nothing(mv):
    """hasEmission is recomputed from the kept cells: one voxel of emission 1 among eight has the mean 0"""
    attribs = X.default_attribs(64)
    attribs[5, 4] = 1
    src, want = check(mv, full(4), attribs, 4, 1)
    assert src.info().hasEmission == 1 and not want["attribs"][:, 4:7].any()
    assert src.coarsen(1, dst=mv.IntersectorOctreeGPU()).info().hasEmission == 0


# ---- exact sums --------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def white_box(mv):
    """264 x 256 x 256 default voxels inside the first 512^3 cell of a 1024^3 grid: 17 301 504 voxels, 4.41e9 per channel"""
    xyz = np.empty((264 * 256 * 256, 3), np.uint32)
    i = np.arange(len(xyz), dtype=np.uint32)
    xyz[:, 0], xyz[:, 1], xyz[:, 2] = i % 264, (i // 264) % 256, i // (264 * 256)
    return build(mv, xyz, 1024)


def test_sums_beyond_32_bits(mv, white_box):
    n = 264 * 256 * 256
    assert n == 17301504 and 255 * n > 2 ** 32 and white_box.info().numberOfVoxels == n
    want = {"xyz": np.zeros((1, 3), np.uint32), "attribs": X.default_attribs(1), "count": np.array([n], np.uint32)}  # (a 32-bit accumulator gives the colour 6)
    assert_listing(white_box, want, 9)
    assert_listing(white_box, want, 9, n)
    assert white_box.coarse_voxels_device(9, n + 1) == 0
    assert_coarsened(mv, white_box, want, n, 1024, 9)
    # and split over the eight cells of k = 8, whose sums stay below 2^32: 256^3 voxels in the first, 8 * 256^2 in the second
    got = white_box.coarse_voxels(8)
    assert got["xyz"].tolist() == [[0, 0, 0], [1, 0, 0]] and got["count"].tolist() == [256 ** 3, 8 * 256 ** 2] and (got["attribs"] == X.default_attribs(2)).all()


# ---- sources of every flavour, edits, fills, uploads ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed():
    rng = np.random.default_rng(40)
    xyz = np.unique(np.concatenate([np.argwhere(rng.random((32, 32, 32)) < 0.3), shell(3, 12)]), axis=0)
    return xyz, random_attribs(rng, len(xyz))


@pytest.mark.parametrize("src_flags", [0, 1, 2, 3])
def test_every_flavour_of_source_and_destination(mv, mixed, src_flags):
    xyz, attribs = mixed
    src, _ = check(mv, xyz, attribs, 32, 2, 1, flags=3 - src_flags, src_flags=src_flags)
    assert src_flags != 3 or src.info().flavour == 2  # the tree flavour is read like any other
    check(mv, xyz, attribs, 32, 1, 2, flags=src_flags, src_flags=src_flags)


def test_after_edits_and_a_fill(mv, mixed):
    xyz, attribs = mixed
    src = build(mv, xyz, 32, 0, attribs)
    rng = np.random.default_rng(41)
    gone = rng.choice(len(xyz), 500, replace=False)
    src.edit_voxels(xyz[gone].astype(np.uint32), None, np.zeros(500, np.uint8))
    added = np.unique(np.concatenate([np.argwhere(rng.random((32, 32, 32)) < 0.01), shell(3, 12)]), axis=0).astype(np.uint32)  # (the shell whole again: a cavity to fill)
    glow = random_attribs(rng, len(added))
    src.edit_voxels(added, glow)
    now_xyz, now_attribs = src.read_voxels()
    assert len(now_xyz) != len(xyz)
    for k in (1, 3):
        want = X.coarse(now_xyz, now_attribs, k)
        assert_listing(src, want, k)
        assert_coarsened(mv, src, want, len(now_xyz), 32, k)
    assert src.fill_enclosed(np.array([1, 2, 3, 4, 5, 6, 7, 8], np.uint8)) > 0
    now_xyz, now_attribs = src.read_voxels()
    want = X.coarse(now_xyz, now_attribs, 2, 3)
    assert_listing(src, want, 2, 3)
    assert_coarsened(mv, src, want, len(now_xyz), 32, 2, 3, flags=1)


def test_an_upload_is_refused_and_works_after_a_rebuild(mv, mixed):
    xyz, attribs = mixed
    built = build(mv, xyz, 32, 0, attribs)
    nodes, attrs, _ = built.download()
    attrs = attrs.copy()
    attrs[:, 3], attrs[:, 7] = 17, np.arange(len(attrs)) % 251  # alpha bytes a voxel-list build never stores: the rebuild keeps them, the coarsening does not read them
    i = built.info()
    up = mv.IntersectorOctreeGPU()
    up.upload(nodes, attrs, LOWER, DPS, 32, i.hasEmission, embeddedMask=bool(i.embeddedMask))
    before = mv.allocation_state()[2]
    with pytest.raises(mv.MvrtError, match="mvrt_svo_coarse_voxels: an uploaded octree keeps no Morton codes"):
        up.coarse_voxels_device(1)
    with pytest.raises(mv.MvrtError, match="mvrt_svo_coarsen: an uploaded octree keeps no Morton codes"):
        up.coarsen(1)
    assert mv.allocation_state()[2] == before
    up.rebuild()
    now_xyz, now_attribs = up.read_voxels()
    assert (now_attribs[:, 3] == 17).all()
    want = X.coarse(now_xyz, now_attribs, 2)
    assert (want["attribs"][:, [3, 7]] == 255).all() and X.same(want, X.coarse(xyz, attribs, 2))
    assert_listing(up, want, 2)
    assert_coarsened(mv, up, want, len(now_xyz), 32, 2)


# ---- destinations ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_in_place_and_over_another_octree(mv, mixed):
    xyz, attribs = mixed
    want = X.coarse(xyz, attribs, 1)
    src = build(mv, xyz, 32, 0, attribs)
    src.set_emission_scale(2.5)
    other = build(mv, full(8), 8, 3)
    other.set_emission_scale(0.75)
    view = bytes(src.device_view())
    assert_coarsened(mv, src, want, len(xyz), 32, 1, dst=other)  # replaced; the emission scale stays the destination's own
    assert other.info().emissionScale == 0.75 and other.info().gridRes == 16 and bytes(src.device_view()) == view
    held = mv.allocation_state()[:2]
    assert_coarsened(mv, src, want, len(xyz), 32, 1, flags=2, dst=src)  # dst == src: the in-place LOD
    assert src.info().emissionScale == 2.5 and src.info().gridRes == 16 and src.info().numberOfVoxels == len(want["xyz"])
    assert mv.allocation_state()[1] < held[1]  # the fine octree is gone
    again = X.coarse(want["xyz"], want["attribs"], 2)  # and down again from there, to the coarsest grid there is
    assert_listing(src, again, 2)
    assert_coarsened(mv, src, X.coarse(want["xyz"], want["attribs"], 3), len(want["xyz"]), 16, 3, dst=src)
    assert src.info().gridRes == 2
    with pytest.raises(mv.MvrtError, match=r"levelsDown 1 is outside \[1, 0\]"):
        src.coarsen(1)


def test_coarsen_through_the_path_tracers_intersector_between_steps(mv):
    """The same two steps around an in-place coarsening and around the build_voxels it stands for: the step issued before finishes first on the fine octree, the
    frame buffer is not cleared, and the second step accumulates on it."""
    tris = bunny_tris()
    v = tris.reshape(-1, 3)
    lo = v.min(0)
    res, w, h = 64, 64, 64
    dps = np.float32((v.max(0) - lo).max() / np.float32(res))
    rgba, hw, hh = mv.read_rgbe_file(os.path.join(GOLDEN, "monks_forest_s.hdr"))
    cam = probe_camera(lo, dps, res, focus=9.0, lens_r=0.05)
    frames = []
    for use_coarsen in (True, False):
        pt = mv.PathTracer()
        pt.setup(None)
        pt.resizeFrameBufferIfNeeded(None, w, h)
        pt.loadHDRIPixels(None, rgba, hw, hh, rgba, hw, hh)
        svo = pt.m_intersectorOctreeGPU
        svo.build(v, None, None, None, lo, dps, res)
        xyz, attribs = svo.read_voxels()
        want = X.coarse(xyz, attribs, 1)
        pt.step(None, cam)
        if use_coarsen:
            svo.coarsen(1)
        else:
            svo.build_voxels(want["xyz"], want["attribs"], origin=lo, dps=np.float32(dps * np.float32(2)), gridRes=res >> 1)
        assert svo.info().numberOfVoxels == len(want["xyz"]) and svo.info().gridRes == 32
        pt.step(None, cam)
        assert pt.getSteps() == 2
        frames.append(pt.read_framebuffer()[: w * h].copy())
        pt.cleanUp()
    assert np.array_equal(frames[0], frames[1]) and frames[0].max() > 0


# ---- the contract of the listing -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(mv, mixed):
    xyz, attribs = mixed
    return build(mv, xyz, 32, 0, attribs), X.coarse(xyz, attribs, 1, 2)


def test_null_outputs(mv, small):
    svo, want = small
    n = len(want["xyz"])
    assert n > 300 and svo.coarse_voxels_device(1, 2) == n  # capacity 0, all NULL
    xyz, attribs, count = mv.DeviceArray((n, 3), np.uint32), mv.DeviceArray((n, 8), np.uint8), mv.DeviceArray(n, np.uint32)
    assert svo.coarse_voxels_device(1, 2, n, xyz, None, None) == n and np.array_equal(xyz.to_host(), want["xyz"])
    assert svo.coarse_voxels_device(1, 2, n, None, attribs, None) == n and np.array_equal(attribs.to_host(), want["attribs"])
    assert svo.coarse_voxels_device(1, 2, n, None, None, count) == n and np.array_equal(count.to_host(), want["count"])
    assert mv.lib().mvrt_svo_coarse_voxels(svo._h, 1, 2, 0, None, None, None, None, None) == 0  # even the count may be NULL
    big, host = filled(mv, (n + 5, 3), np.uint32)  # a larger capacity than the count is fine and writes the count's worth
    assert svo.coarse_voxels_device(1, 2, n + 5, big, None, None) == n
    assert np.array_equal(big.to_host()[:n], want["xyz"]) and np.array_equal(big.to_host()[n:], host[n:])


@pytest.mark.parametrize("min_count", [1, 2])
def test_capacity_one_short(mv, small, mixed, min_count):
    svo = small[0]
    n = len(X.coarse(mixed[0], mixed[1], 1, min_count)["xyz"])
    (xyz, xyz_host), (attribs, attribs_host), (count, count_host) = filled(mv, (n, 3), np.uint32), filled(mv, (n, 8), np.uint8), filled(mv, n, np.uint32)
    lib = mv.lib()
    got = C.c_uint64(0)
    assert lib.mvrt_svo_coarse_voxels(svo._h, 1, min_count, n - 1, xyz.ptr, attribs.ptr, count.ptr, C.byref(got), None) != 0
    assert got.value == n and b"capacity %d" % (n - 1) in lib.mvrt_last_error() and b"%d coarse voxels" % n in lib.mvrt_last_error()
    assert np.array_equal(xyz.to_host(), xyz_host) and np.array_equal(attribs.to_host(), attribs_host) and np.array_equal(count.to_host(), count_host)  # nothing was written
    with pytest.raises(mv.MvrtError, match="capacity"):
        svo.coarse_voxels_device(1, min_count, n - 1, None, None, count)
    assert np.array_equal(count.to_host(), count_host)


def test_refusals_without_gpu_work(mv, small):
    svo = small[0]
    empty, dst = mv.IntersectorOctreeGPU(), mv.IntersectorOctreeGPU()
    before = mv.allocation_state()[2]
    for call, who in ((lambda h, k, m: h.coarse_voxels_device(k, m), "mvrt_svo_coarse_voxels"), (lambda h, k, m: h.coarsen(k, m, 0, dst), "mvrt_svo_coarsen")):
        for h, k, m, text in ((empty, 1, 1, "no octree"), (svo, 0, 1, r"levelsDown 0 is outside \[1, "), (svo, -1, 1, r"levelsDown -1 is outside \[1, "),
                              (svo, 5, 1, r"levelsDown 5 is outside \[1, 4\]"), (svo, 6, 1, r"levelsDown 6 is outside \[1, 4\]"), (svo, 1, 0, "minCount 0 is outside"),
                              (svo, 1, 9, r"minCount 9 is outside \[1, 8\^levelsDown = 8\]"), (svo, 4, 4097, r"minCount 4097 is outside \[1, 8\^levelsDown = 4096\]")):
            with pytest.raises(mv.MvrtError, match=who + ": " + text):
                call(h, k, m)
    for flags in (4, 16):
        with pytest.raises(mv.MvrtError, match="mvrt_svo_coarsen: unsupported flags"):
            svo.coarsen(1, 1, flags, dst)
    assert mv.allocation_state()[2] == before and dst.info().numberOfNodes == 0
    assert svo.coarse_voxels_device(4, 4096) == 0  # the largest legal minCount of the coarsest level: no cell of this set is full


def test_the_handle_is_not_modified(mv, small):
    svo, want = small
    before = svo.download(want_morton=True)
    info = bytes(svo.info())
    view = bytes(svo.device_view())
    held = mv.allocation_state()[:2]
    assert_listing(svo, want, 1, 2)
    assert bytes(svo.info()) == info and bytes(svo.device_view()) == view and all(np.array_equal(a, b) for a, b in zip(svo.download(want_morton=True), before))
    assert mv.allocation_state()[:2] == held  # the scratch is gone


def test_a_voxel_size_that_leaves_fp32_is_refused(mv):
    src = build(mv, full(4), 4, dps=np.float32(3.0e38))  # dps * 2 is +inf
    held, info = src.download(want_morton=True), bytes(src.info())
    for dst in (src, mv.IntersectorOctreeGPU()):
        with pytest.raises(mv.MvrtError, match="mvrt_svo_coarsen: dps .* is not finite"):
            src.coarsen(1, dst=dst)
        assert dst is src or dst.info().numberOfNodes == 0
    assert bytes(src.info()) == info and all(np.array_equal(a, b) for a, b in zip(src.download(want_morton=True), held))
    assert src.coarse_voxels_device(1) == 8  # the listing has no voxel size to refuse
