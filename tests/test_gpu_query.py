"""The nearest voxel of arbitrary lattice points on the GPU (mvrt_svo_nearest_voxels / mvrt_svo_nearest_between / mvrt_svo_transfer_attributes)
against the numpy model of tests/query_expected.py, which takes the minimum of ( d2, vIndex ) over all voxels by brute force and knows nothing of the descent:
dist2, nearest and attribs bit for bit, on the smallest shapes that can break each mechanism -- one voxel, the bisector plane, a cube shell with every cell and a
ring of outside points at query counts around the wave, the sphere shell at its centre (mass ties), the corners of the 2^21 grid, the 21-level path, the bunny
with its own voxels -- then the flavours, edits and uploads, the limit at its boundary values, the two-set call with its summary and the transfer against a twin
handle given edit_voxels with the model's attributes."""
import numpy as np
import pytest

import query_expected as Q
import surface_expected as S
from common import bunny_tris
from fixtures import mv  # noqa: F401 (fixtures)
from voxel_sets import DPS, LOWER, colours, filled, full, octree, same, shell

pytestmark = pytest.mark.gpu

KEYS = ("dist2", "nearest", "attribs")
NO_LIMIT, NONE = Q.NO_LIMIT, Q.NONE


def build(mv, xyz, res, flags=0, attribs=None, emission=True, seed=1):
    xyz = np.ascontiguousarray(xyz, np.uint32).reshape(-1, 3)
    svo = mv.IntersectorOctreeGPU()
    svo.build_voxels(xyz, colours(len(xyz), seed, emission) if attribs is None else attribs, origin=LOWER, dps=DPS, gridRes=res, flags=flags)
    return svo


def ask(svo, queries, max_dist2=NO_LIMIT):
    """the answers of the handle against the model on the voxels the handle holds; -> the model's"""
    x0, a0 = svo.read_voxels()
    want = Q.nearest_voxels(x0, a0, queries, max_dist2)
    got = svo.nearest_voxels(queries, max_dist2)
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    return want


# ---- the walk -------------------------------------------------------------------------------------------------------------------------------------------------
def test_one_voxel_and_the_bisector_plane(mv):
    svo = build(mv, [(5, 2, 9)], 16)
    q = np.array([(5, 2, 9), (0, 0, 0), (15, 15, 15), (-40, 3, 60), (5, 2, 10)], np.int32)
    want = ask(svo, q)
    assert want["dist2"].tolist() == [0, 25 + 4 + 81, 100 + 169 + 36, 45 * 45 + 1 + 51 * 51, 1] and (want["nearest"] == 0).all()
    svo = build(mv, [(3, 8, 8), (11, 8, 8)], 16)  # the plane x = 7: every point of it is as far from the one as from the other
    plane = np.array([(7, y, z) for y in (-3, 0, 8, 15, 20) for z in (-9, 8, 15)], np.int32)
    want = ask(svo, plane)
    assert (want["nearest"] == 0).all()  # (3, 8, 8) has the lower code
    assert ask(svo, plane + (1, 0, 0))["nearest"].tolist() == [1] * len(plane)


@pytest.fixture(scope="module")
def cube_case(mv):
    svo = build(mv, shell(4, 11), 16)  # a 7^3 cube shell
    ring = np.array([(x, y, z) for x in (-9, 3, 8, 24) for y in (-1, 7, 16) for z in (-17, 5, 40)], np.int32)
    return svo, np.concatenate([full(16).astype(np.int32), ring])


def test_cube_shell_every_cell_and_a_ring_outside(mv, cube_case):
    svo, q = cube_case
    want = ask(svo, q)
    assert len(q) == 4096 + 36 and (want["dist2"][:4096] == 0).sum() == 7 ** 3 - 5 ** 3 and want["dist2"].max() > 17 * 17
    stats = mv.nearest_query_stats()
    print("cube shell:", stats)
    assert stats["queries"] == len(q) and stats["visits"] >= len(q) and stats["most"] >= 2 and stats["compared"] >= len(q)


@pytest.mark.parametrize("count", [1, 63, 64, 65, 255, 257])
def test_query_counts_around_the_wave(mv, cube_case, count):
    svo, q = cube_case
    ask(svo, q[np.random.default_rng(count).permutation(len(q))[:count]])


def test_no_query_is_a_success_without_a_launch(mv, cube_case):
    svo = cube_case[0]
    allocs = mv.allocation_state()[2]
    got = svo.nearest_voxels(np.zeros((0, 3), np.int32))
    assert all(len(got[k]) == 0 for k in KEYS) and mv.allocation_state()[2] == allocs
    assert mv.nearest_query_stats() == {"queries": 0, "visits": 0, "most": 0, "compared": 0}


def test_sphere_shell_mass_ties_at_the_centre(mv):
    p = full(32) - 16
    r2 = (p * p).sum(1)
    svo = build(mv, (p + 16)[(r2 <= 13 * 13) & (r2 > 12 * 12)], 32)
    for q in ([(16, 16, 16)], [(17, 16, 16)], [(16, 15, 16)]):
        want = ask(svo, np.array(q, np.int32))
        print("sphere shell of", svo.info().numberOfVoxels, "voxels from", q, "d2", int(want["dist2"][0]), mv.nearest_query_stats())
        assert want["dist2"][0] > 11 * 11


def test_corners_of_the_largest_grid_and_the_21_level_path(mv):
    res, m = 1 << 21, 1 << 22
    svo = build(mv, [(0, 0, 0), (res - 1, res - 1, res - 1)], res)
    q = np.array([(0, 0, 0), (res - 1,) * 3, (res - 1, 0, 0), (0, res - 1, res - 1), (-m, -m, -m), (m, m, m), (m, -m, m), (res // 2 - 1,) * 3, (res // 2,) * 3], np.int32)
    want = ask(svo, q)
    assert want["nearest"].tolist() == [0, 1, 0, 1, 0, 1, 1, 0, 1] and want["dist2"][4] == 3 << 44
    svo = build(mv, [(res - 1, res - 1, res - 1)], res)  # one voxel below 21 levels
    want = ask(svo, np.array([(0, 0, 0), (res - 1,) * 3, (-m, -m, -m), (m, -m, 5)], np.int32))
    assert want["dist2"][2] == 3 * (m + res - 1) ** 2 and (1 << 46) < want["dist2"][2] < (1 << 47)


@pytest.fixture(scope="module")
def bunny_case(mv):
    v = bunny_tris().reshape(-1, 3)
    lo = v.min(0)
    dps = np.float32((v.max(0) - lo).max() / np.float32(64))
    base = mv.IntersectorOctreeGPU()
    base.build(v, None, None, None, lo, dps, 64)
    x0, _ = base.read_voxels()
    svo = mv.IntersectorOctreeGPU()
    svo.build_voxels(x0, colours(len(x0), 12), origin=lo, dps=dps, gridRes=64)
    x0, a0 = svo.read_voxels()
    shifted = x0.astype(np.int32) + np.array((3, -2, 5), np.int32)
    return svo, x0, a0, shifted, Q.nearest_voxels(x0, a0, shifted)


def test_bunny_at_64_with_its_own_voxels(mv, bunny_case):
    svo, x0, a0, shifted, want = bunny_case
    got = svo.nearest_voxels(x0.astype(np.int32))
    assert len(x0) == 8516 and (got["dist2"] == 0).all() and np.array_equal(got["nearest"], np.arange(len(x0), dtype=np.uint32)) and np.array_equal(got["attribs"], Q.alpha255(a0))
    got = svo.nearest_voxels(shifted)
    print("bunny shifted by (3, -2, 5):", mv.nearest_query_stats(), "deepest", int(want["dist2"].max()))
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), k
    assert want["dist2"].max() > 9


def test_limit_at_zero_and_at_the_boundary_values(mv, bunny_case):
    svo, x0, a0, shifted, want = bunny_case
    d2 = np.sort(np.unique(want["dist2"]))
    mid = int(d2[len(d2) // 2])
    for limit in (0, mid - 1, mid, mid + 1, int(d2[-1]), NO_LIMIT - 1):
        got = svo.nearest_voxels(shifted, limit)
        within = want["dist2"] <= limit
        assert within.any() and (limit >= int(d2[-1]) or not within.all())
        for k in KEYS:
            assert np.array_equal(got[k][within], want[k][within]), (limit, k)  # the limit never changes an answer that lies within it
        assert (got["dist2"][~within] == NO_LIMIT).all() and (got["nearest"][~within] == NONE).all() and not got["attribs"][~within].any()
    member = svo.nearest_voxels(np.concatenate([x0[:50].astype(np.int32), shifted[:50]]), 0)  # 0 is the membership test
    assert (member["dist2"][:50] == 0).all() and np.array_equal(member["dist2"][50:] == 0, want["dist2"][:50] == 0)


def test_any_output_may_be_null(mv, cube_case):
    svo, q = cube_case
    x0, a0 = svo.read_voxels()
    want = Q.nearest_voxels(x0, a0, q)
    qd = mv.DeviceArray.from_host(q)
    shapes = {"dist2": (len(q), np.uint64), "nearest": (len(q), np.uint32), "attribs": ((len(q), 8), np.uint8)}
    for k in KEYS:
        out = mv.DeviceArray(*shapes[k])
        svo.nearest_voxels_device(len(q), qd, **{k: out})
        assert np.array_equal(out.to_host(), want[k]), k
    svo.nearest_voxels_device(len(q), qd)  # none at all: only the figures
    assert mv.nearest_query_stats()["queries"] == len(q)


# ---- flavours, edits, uploads ---------------------------------------------------------------------------------------------------------------------------------
def scattered(res=16, percent=5, seed=3):
    p = full(res)
    return p[np.random.default_rng(seed).random(len(p)) * 100 < percent]


def probes(res, n=300, seed=4):
    return np.random.default_rng(seed).integers(-6, res + 6, size=(n, 3)).astype(np.int32)


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_every_flavour(mv, flags):
    svo = build(mv, scattered(), 16, flags)
    assert flags != 3 or svo.info().flavour == 2
    before = octree(svo)
    ask(svo, probes(16))
    assert same(octree(svo), before)  # the handle is never modified


def test_after_an_edit_and_a_rebuilt_upload(mv):
    svo = build(mv, scattered(), 16)
    svo.edit_voxels(np.array([(7, 7, 7), (1, 1, 1)], np.uint32), colours(2, 8))
    svo.edit_voxels(scattered()[:5].astype(np.uint32), None, np.zeros(5, np.uint8))
    want = ask(svo, probes(16))
    nodes, attrs, _ = svo.download()
    i = svo.info()
    up = mv.IntersectorOctreeGPU()
    up.upload(nodes, attrs, LOWER, DPS, 16, i.hasEmission, embeddedMask=bool(i.embeddedMask))
    allocs = mv.allocation_state()[2]
    for call in (lambda: up.nearest_voxels(probes(16)), lambda: up.nearest_between(svo), lambda: svo.nearest_between(up), lambda: up.transfer_attributes(svo),
                 lambda: svo.transfer_attributes(up)):
        with pytest.raises(mv.MvrtError, match="keeps no Morton codes"):
            call()
    assert mv.allocation_state()[2] == allocs
    up.rebuild()
    got = up.nearest_voxels(probes(16))
    assert all(np.array_equal(got[k], want[k]) for k in KEYS)


def test_refusals_without_gpu_work(mv, cube_case):
    svo = cube_case[0]
    empty = mv.IntersectorOctreeGPU()
    allocs = mv.allocation_state()[2]
    for call in (lambda: empty.nearest_voxels(probes(16)), lambda: empty.nearest_between(svo), lambda: svo.nearest_between(empty), lambda: empty.transfer_attributes(svo),
                 lambda: svo.transfer_attributes(empty)):
        with pytest.raises(mv.MvrtError, match="no octree"):
            call()
    for offset in ((0, (1 << 21) + 1, 0), (-(1 << 21) - 1, 0, 0)):
        with pytest.raises(mv.MvrtError, match="offset"):
            svo.nearest_between(svo, offset)
        with pytest.raises(mv.MvrtError, match="offset"):
            svo.transfer_attributes(svo, offset)
    for flags in (0, 4, 7, 1 << 31):
        with pytest.raises(mv.MvrtError, match="flags"):
            svo.transfer_attributes(svo, flags=flags)
    with pytest.raises(mv.MvrtError, match="2\\^32"):
        svo.nearest_voxels_device(1 << 32, 8)
    assert mv.allocation_state()[2] == allocs


# ---- two sets -------------------------------------------------------------------------------------------------------------------------------------------------
def assert_between(mv, a, b, offset=None, max_dist2=NO_LIMIT):
    xa, xb = a.read_voxels()[0], b.read_voxels()[0]
    want = Q.nearest_between(xa, xb, (0, 0, 0) if offset is None else offset, max_dist2)
    got = a.nearest_between(b, offset, max_dist2)
    for k in ("dist2", "nearest"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    for k in ("n", "maxDist2", "farthest", "zero", "beyond"):
        assert got[k] == want[k], (k, got[k], want[k])
    summary = a.nearest_between_device(b, offset, max_dist2)  # both arrays None
    assert summary == {k: want[k] for k in ("n", "maxDist2", "farthest", "zero", "beyond")}
    return want


def test_cube_against_shifted_cube_and_grids_of_different_size(mv, cube_case):
    a = cube_case[0]
    b = build(mv, shell(4, 11) + (2, 0, 1), 16, seed=2)
    want = assert_between(mv, a, b)
    assert want["maxDist2"] == 5 and 0 < want["zero"] < want["n"] and want["beyond"] == 0
    assert assert_between(mv, a, b, (-2, 0, -1))["zero"] == want["n"]  # moved back: the same cube
    want = assert_between(mv, a, b, (1, -3, 0), 4)
    assert want["beyond"] > 0 and want["maxDist2"] <= 4
    assert assert_between(mv, a, b, (9, 9, 9), 3)["beyond"] == want["n"]  # every voxel beyond: no farthest one
    big = build(mv, shell(4, 11) * 3 + 40, 128, seed=5)  # gridRes 128 against 16, nothing is clipped
    assert assert_between(mv, a, big, (-30, 0, 0))["maxDist2"] > 40 * 40
    assert_between(mv, big, a, (1 << 21, -(1 << 21), 0))


def test_a_set_against_itself(mv, bunny_case):
    svo = bunny_case[0]
    got = svo.nearest_between(svo)
    n = svo.info().numberOfVoxels
    assert (got["dist2"] == 0).all() and np.array_equal(got["nearest"], np.arange(n, dtype=np.uint32))
    assert (got["n"], got["maxDist2"], got["farthest"], got["zero"], got["beyond"]) == (n, 0, 0, n, 0)
    want = bunny_case[4]  # the bunny's voxels moved by (3, -2, 5) asked in the bunny: a against a - o with o = -(3, -2, 5)
    got = svo.nearest_between(svo, (-3, 2, -5))
    assert np.array_equal(got["dist2"], want["dist2"]) and np.array_equal(got["nearest"], want["nearest"])
    assert got["maxDist2"] == want["dist2"].max() and got["farthest"] == np.flatnonzero(want["dist2"] == want["dist2"].max())[0]


def test_capacity_too_small_writes_nothing(mv, cube_case):
    a = cube_case[0]
    n = a.info().numberOfVoxels
    d2, hd = filled(mv, n, np.uint64)
    near, hn = filled(mv, n, np.uint32)
    for arrays in ({"dist2": d2, "nearest": near}, {"dist2": d2}, {"nearest": near}):
        with pytest.raises(mv.MvrtError, match="capacity %d is smaller than the %d" % (n - 1, n)):
            a.nearest_between_device(a, capacity=n - 1, **arrays)
        assert np.array_equal(d2.to_host(), hd) and np.array_equal(near.to_host(), hn)
    assert a.nearest_between_device(a, capacity=n, dist2=d2)["zero"] == n and not d2.to_host().any() and np.array_equal(near.to_host(), hn)


@pytest.mark.parametrize("offset", [(0, 0, 0), (1, 0, 0), (-2, 3, 1)])
def test_zero_count_equals_the_overlap_of_combine(mv, cube_case, offset):
    a = cube_case[0]
    b = build(mv, np.unique(np.concatenate([shell(5, 12), scattered()]), axis=0), 16, seed=2)
    assert a.nearest_between_device(b, offset)["zero"] == a.combine_voxels(b, mv.COMBINE_INTERSECTION, offset)["overlap"] > 0


# ---- transfer -------------------------------------------------------------------------------------------------------------------------------------------------
def with_odd_alphas(mv, svo, res, seed=9):
    """the same voxels with random alpha bytes: build_voxels stores 255 itself, an upload carries its bytes verbatim and a rebuild keeps them"""
    nodes, attrs, _ = svo.download()
    i = svo.info()
    attrs = attrs.copy()
    attrs[:, 3], attrs[:, 7] = np.random.default_rng(seed).integers(0, 255, (2, len(attrs)), dtype=np.uint8)
    up = mv.IntersectorOctreeGPU()
    up.upload(nodes, attrs, LOWER, DPS, res, i.hasEmission, embeddedMask=bool(i.embeddedMask))
    up.rebuild()
    assert np.array_equal(up.read_voxels()[1], attrs)
    return up


def assert_transfer(mv, dst_xyz, src, res, offset=None, max_dist2=NO_LIMIT, flags=3, dst_emission=False, seed=7, odd=False):
    """dst after the transfer == a twin given edit_voxels with the model's attributes for the voxels within the limit"""
    dst, twin = build(mv, dst_xyz, res, emission=dst_emission, seed=seed), build(mv, dst_xyz, res, emission=dst_emission, seed=seed)
    if odd:
        dst, twin = with_odd_alphas(mv, dst, res), with_odd_alphas(mv, twin, res)
    xs, as_ = src.read_voxels()
    xd, ad = dst.read_voxels()
    x, new, taken, changed = Q.transferred(xd, ad, xs, as_, (0, 0, 0) if offset is None else offset, max_dist2, flags)
    if taken.any() and changed:
        twin.edit_voxels(x[taken].astype(np.uint32), new[taken])
    got = dst.transfer_attributes(src, offset, max_dist2, flags)
    assert got == (changed, int((~taken).sum()))
    assert same(octree(dst), octree(twin)) and same(dst.read_voxels(), twin.read_voxels()) and np.array_equal(dst.read_voxels()[1], new)
    assert bytes(dst.info()) == bytes(twin.info())
    return dst, taken, changed


@pytest.mark.parametrize("flags", [1, 2, 3])
def test_transfer_equals_an_edit_with_the_models_attributes(mv, cube_case, flags):
    src = build(mv, scattered(16, 8, 9), 16, seed=3)
    dst, taken, changed = assert_transfer(mv, shell(4, 11), src, 16, (1, 0, -1), flags=flags)
    assert taken.all() and changed == len(taken)


def test_transfer_with_a_limit_leaves_the_rest_verbatim(mv):
    src = build(mv, scattered(16, 2, 9), 16, seed=3)
    dst, taken, changed = assert_transfer(mv, shell(3, 13), src, 16, None, 6, dst_emission=True, odd=True)
    assert 0 < taken.sum() < len(taken) and changed == taken.sum()  # (every voxel taken loses its odd alphas at least)
    alphas = dst.read_voxels()[1][:, [3, 7]]
    assert (alphas[taken] == 255).all() and (alphas[~taken] != 255).all(1).any()  # the others byte for byte, odd alphas included


def test_transfer_turns_emission_on_and_off(mv):
    lit, dark = build(mv, scattered(16, 8, 9), 16, seed=3), build(mv, scattered(16, 8, 9), 16, emission=False, seed=3)
    dst, _, _ = assert_transfer(mv, shell(4, 11), lit, 16, flags=2, dst_emission=False)
    assert dst.info().hasEmission == 1
    dst, _, _ = assert_transfer(mv, shell(4, 11), dark, 16, flags=2, dst_emission=True)
    assert dst.info().hasEmission == 0
    dst, _, _ = assert_transfer(mv, shell(4, 11), dark, 16, flags=1, dst_emission=True)
    assert dst.info().hasEmission == 1  # the emission word is the voxel's own


def test_transfer_that_changes_nothing_leaves_the_views_valid(mv):
    at = colours(len(shell(4, 11)), 5)
    at[:, 3] = at[:, 7] = 255
    dst = build(mv, shell(4, 11), 16, attribs=at)
    far = build(mv, [(0, 0, 0)], 16)
    view, before, allocs = dst.device_view(), octree(dst), mv.allocation_state()[:2]
    assert dst.transfer_attributes(dst) == (0, 0)  # itself, alphas already 255
    assert dst.transfer_attributes(far, (0, 0, 0), 2) == (0, dst.info().numberOfVoxels)  # everything beyond the limit
    after = dst.device_view()
    assert bytes(after) == bytes(view) and same(octree(dst), before) and mv.allocation_state()[:2] == allocs


def test_transfer_from_itself(mv):
    xyz = shell(4, 11)
    dst = with_odd_alphas(mv, build(mv, xyz, 16), 16)
    x0, a0 = dst.read_voxels()
    changed, beyond = dst.transfer_attributes(dst)
    assert beyond == 0 and changed == int((Q.alpha255(a0) != a0).any(1).sum()) > 0 and np.array_equal(dst.read_voxels()[1], Q.alpha255(a0))  # o = 0: only the alphas
    assert_transfer(mv, xyz, build(mv, xyz, 16, seed=7), 16, (2, 1, 0))  # (the same bytes as dst: what dst == src with an offset must give)
    dst = build(mv, xyz, 16, seed=7)
    _, new, _, changed = Q.transferred(*dst.read_voxels(), *dst.read_voxels(), (2, 1, 0))
    assert dst.transfer_attributes(dst, (2, 1, 0)) == (changed, 0) and np.array_equal(dst.read_voxels()[1], new)  # near is taken before anything is written


# ---- the engines that answer in special places ----------------------------------------------------------------------------------------------------------------------
def test_agreement_with_enclosed_nearest_and_the_distance_band(mv):
    p = full(24)
    rng = np.random.default_rng(6)
    svo = build(mv, np.concatenate([shell(3, 21), (p[(p > 3).all(1) & (p < 20).all(1)])[rng.random(16 ** 3) < 0.02]]), 32)
    for listing in (svo.enclosed_nearest(), svo.distance_cells(1024)):
        assert len(listing["xyz"]) > 1000
        got = svo.nearest_voxels(listing["xyz"].astype(np.int32))
        assert np.array_equal(got["dist2"], listing["dist2"].astype(np.uint64)) and np.array_equal(got["nearest"], listing["nearest"]) and np.array_equal(got["attribs"], listing["attribs"])
