"""Boolean operations between two voxel sets on the GPU (mvrt_svo_combine_voxels / mvrt_svo_combine) against the model of tests/combine_expected.py, bit for
bit: the listing array by array, the in-place call through read_voxels, the identity with the edit through a twin handle that was given the model's SET / REMOVE
lists via edit_voxels.  On the smallest inputs that can break each mechanism -- gridRes 2 with one voxel each, a list of one, the workgroup seam at 255 / 256 /
257 voxels, B' entirely below and above A, identical sets, the 3-D checkerboard split by parity, random sets, offsets that clip nothing, a layer and everything,
the borders of the 2^21 grid, grids of different size, a == b, the attribute flag, alpha bytes of b, every flavour, edited / filled / closed / pruned / rebuilt
handles, steps in flight, the bunny -- and the contract of the two calls."""
import ctypes as C
import os

import numpy as np
import pytest

import combine_expected as E
import surface_expected as S
from common import GOLDEN, bunny_tris, probe_camera
from fixtures import load
from voxel_sets import DPS, LOWER, assert_same_octree, build, colours, filled, full, octree, same, specks_and_block

pytestmark = pytest.mark.gpu

REMOVE = 0  # IntersectorOctreeGPU.VOXEL_REMOVE


@pytest.fixture(scope="module")
def mv():
    m = load()
    assert (m.COMBINE_UNION, m.COMBINE_INTERSECTION, m.COMBINE_DIFFERENCE, m.COMBINE_XOR, m.COMBINE_ATTRIB_B) == (E.UNION, E.INTERSECTION, E.DIFFERENCE, E.XOR, E.ATTRIB_B)
    return m


def assert_listing(a, b, op, offset=None, flags=0):
    """the listing against the model, array by array; returns the model's result"""
    (xa, aa), (xb, ab) = a.read_voxels(), b.read_voxels()
    res = int(a.info().gridRes)
    want, got = E.combine(xa, aa, xb, ab, res, op, offset, flags), a.combine_voxels(b, op, offset, flags)
    n = len(want["xyz"])
    print("op", op, "offset", offset, "flags", flags, "|A|", len(xa), "|B|", len(xb), "n", len(got["xyz"]), "model", n, "overlap", got["overlap"], "model", want["overlap"],
          "clipped", got["clipped"], "model", want["clipped"])
    assert a.combine_voxels_device(b, op, offset, flags) == (n, want["overlap"], want["clipped"])  # the sizing call
    assert (got["overlap"], got["clipped"]) == (want["overlap"], want["clipped"])
    assert got["xyz"].dtype == np.uint32 and got["xyz"].shape == (n, 3) and np.array_equal(got["xyz"], want["xyz"])
    assert got["attribs"].dtype == np.uint8 and got["attribs"].shape == (n, 8) and np.array_equal(got["attribs"], want["attribs"])
    assert got["source"].dtype == np.uint8 and got["source"].shape == (n,) and np.array_equal(got["source"], want["source"])
    return want


def assert_in_place(mv, a, b, op, offset=None, flags=0, build_flags=None):
    """one in-place call on the handle a against the model and against the edit it stands for; a is modified"""
    (xa, aa), (xb, ab) = a.read_voxels(), b.read_voxels()
    res = int(a.info().gridRes)
    want = E.combine(xa, aa, xb, ab, res, op, offset, flags)
    ex, eat, eops, (added, removed) = E.edit_lists(xa, aa, xb, ab, res, op, offset, flags)
    before, info, b_before, b_info = octree(a), bytes(a.info()), octree(b), bytes(b.info())
    if len(want["xyz"]) == 0:
        with pytest.raises(mv.MvrtError, match="would leave no voxel"):
            a.combine(b, op, offset, flags)
        assert bytes(a.info()) == info and same(octree(a), before) and bytes(b.info()) == b_info and same(octree(b), b_before)
        return a
    twin = mv.IntersectorOctreeGPU()
    i = a.info()
    twin.build_voxels(xa, aa, origin=np.array(i.lower[:], np.float32), dps=np.float32(i.dps), gridRes=res, flags=build_flags if build_flags is not None else 0)
    twin.set_emission_scale(i.emissionScale)
    if not np.array_equal(twin.read_voxels()[1], aa):  # bytes a build does not keep (the alpha of a filled cell): an attribute-only edit cannot give them either
        twin = None
    got = a.combine(b, op, offset, flags)
    gx, ga = a.read_voxels()
    print("in place op", op, "offset", offset, "flags", flags, "|A|", len(xa), "->", len(gx), "model", len(want["xyz"]), "added / removed / clipped", got, "model",
          (added, removed, want["clipped"]), "edit entries", len(ex))
    recolour_only = added == 0 and removed == 0 and len(ex) > 0
    assert got == (added, removed, want["clipped"])
    assert np.array_equal(gx, want["xyz"]) and np.array_equal(ga, want["attribs"]) and a.info().numberOfVoxels == len(want["xyz"])
    if a is not b:
        assert bytes(b.info()) == b_info and same(octree(b), b_before)
    if len(ex) == 0:  # nothing changes: the handle is not touched
        assert bytes(a.info()) == info and same(octree(a), before)
        return a
    assert a.info().hasEmission == int(want["attribs"][:, 4:7].any()) and a.info().totalDumpedVoxels == 0
    if recolour_only:
        assert same(octree(a)[:1], before[:1])  # the nodes
    if twin is not None:
        twin.edit_voxels(ex, eat, eops)
        assert_same_octree(a, twin)
    return a


def assert_all(mv, xa, xb, res, offset=None, res_b=None, flags=(0, E.ATTRIB_B), ops=E.OPS, build_flags=0, build_flags_b=0):
    """every op and flag on fresh builds of the two sets: the listing and the in-place call"""
    b = build(mv, xb, res if res_b is None else res_b, build_flags_b, seed=2)
    reader = build(mv, xa, res, build_flags)
    out = {}
    for op in ops:
        for f in flags:
            out[op, f] = assert_listing(reader, b, op, offset, f)
            assert_in_place(mv, build(mv, xa, res, build_flags), b, op, offset, f, build_flags)
    return out


def first_codes(n, res, start=0):
    """the cells with the Morton codes start .. start + n - 1"""
    return S.decode(np.arange(start, start + n, dtype=np.uint64))


# ---- the smallest inputs -----------------------------------------------------------------------------------------------------------------------------------------
def test_grid_res_2_one_voxel_each(mv):
    same_cell = assert_all(mv, [(1, 0, 1)], [(1, 0, 1)], 2)
    assert [len(same_cell[op, 0]["xyz"]) for op in E.OPS] == [1, 1, 0, 0]
    other_cell = assert_all(mv, [(1, 0, 1)], [(0, 1, 1)], 2)
    assert [len(other_cell[op, 0]["xyz"]) for op in E.OPS] == [2, 0, 1, 2]
    moved = assert_all(mv, [(1, 0, 1)], [(0, 1, 1)], 2, offset=(1, -1, 0))  # ... onto the same cell
    assert [len(moved[op, 0]["xyz"]) for op in E.OPS] == [1, 1, 0, 0]


@pytest.mark.parametrize("n", [255, 256, 257])
def test_a_list_of_one_and_the_workgroup_seam(mv, n):
    many = first_codes(n, 16)
    for k in (0, 127, n - 2, n - 1, n, 300):  # the single voxel at the start, inside, at the last two places of the list, right behind it and further on
        one = first_codes(1, 16, k)
        assert_all(mv, many, one, 16, flags=(E.ATTRIB_B,))
        assert_all(mv, one, many, 16, flags=(0,))
    # two lists across the seam that interleave: even against odd codes, and against themselves shifted by one code
    both = first_codes(2 * n, 16)
    assert_all(mv, both[0::2], both[1::2], 16, flags=(0,))
    assert_all(mv, both[:n], both[n - 1:], 16)


def test_b_entirely_below_and_above_a(mv):
    low, high = first_codes(300, 16, 0), first_codes(300, 16, 2000)
    for xa, xb in ((high, low), (low, high)):
        out = assert_all(mv, xa, xb, 16)
        assert out[E.UNION, 0]["overlap"] == 0 and len(out[E.UNION, 0]["xyz"]) == 600
    # touching: the last code of one is the first of the other
    assert_all(mv, first_codes(300, 16, 0), first_codes(300, 16, 299), 16)


def test_identical_sets(mv):
    xyz = np.argwhere(np.random.default_rng(3).random((16, 16, 16)) < 0.3)
    a, b = build(mv, xyz, 16), build(mv, xyz, 16, seed=5)
    view, before, info, held = bytes(a.device_view()), octree(a), bytes(a.info()), mv.allocation_state()[:2]
    for op in E.OPS:
        want = assert_listing(a, b, op)
        assert len(want["xyz"]) == (len(xyz) if op in (E.UNION, E.INTERSECTION) else 0) and want["overlap"] == len(xyz)
    assert a.combine(b, E.UNION) == (0, 0, 0) and a.combine(b, E.INTERSECTION) == (0, 0, 0)
    assert a.combine(a, E.UNION) == (0, 0, 0)
    assert bytes(a.device_view()) == view and bytes(a.info()) == info and same(octree(a), before)
    assert mv.allocation_state()[:2] == held  # the same arrays at the same addresses: no rebuild
    for op in (E.DIFFERENCE, E.XOR):
        with pytest.raises(mv.MvrtError, match="would leave no voxel"):
            a.combine(b, op)
        with pytest.raises(mv.MvrtError, match="would leave no voxel"):
            a.combine(a, op, flags=E.ATTRIB_B)
    assert bytes(a.device_view()) == view and bytes(a.info()) == info and same(octree(a), before) and mv.allocation_state()[:2] == held


# ---- ranks across waves and workgroups ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [8, 16])
def test_checkerboard_split_by_parity(mv, res):
    even = np.argwhere(np.indices((res,) * 3).sum(0) % 2 == 0)
    odd = np.argwhere(np.indices((res,) * 3).sum(0) % 2 == 1)
    out = assert_all(mv, even, odd, res, flags=(0,))
    assert len(out[E.UNION, 0]["xyz"]) == res ** 3 and out[E.UNION, 0]["overlap"] == 0
    assert np.array_equal(out[E.UNION, 0]["xyz"], S.decode(np.arange(res ** 3, dtype=np.uint64)))
    out = assert_all(mv, even, even, res, offset=(1, 0, 0), flags=(0,), ops=(E.UNION, E.XOR))  # the shifted board is the other parity, one layer clipped
    assert out[E.UNION, 0]["clipped"] == res * res // 2 and out[E.UNION, 0]["overlap"] == 0


@pytest.fixture(scope="module")
def random_pair():
    rng = np.random.default_rng(17)
    a = rng.random((32, 32, 32)) < 0.2
    b = np.where(rng.random((32, 32, 32)) < 0.5, a, rng.random((32, 32, 32)) < 0.2)  # about half of b lies on a
    return np.argwhere(a), np.argwhere(b)


def test_random_sets(mv, random_pair):
    xa, xb = random_pair
    out = assert_all(mv, xa, xb, 32)
    assert len(xa) > 5000 and 0.3 * len(xb) < out[E.UNION, 0]["overlap"] < 0.8 * len(xb)


# ---- the offset -----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [(0, 0, 0), (1, 0, 0), (0, -1, 0), (-3, 2, -1), (0, 0, 31), (0, 32, 0), (-32, 0, 0), (40, -40, 5)])
def test_offsets_that_clip_nothing_a_layer_and_everything(mv, offset):
    g = np.zeros((32, 32, 32), bool)
    g[1:31, 1:31, 1:31] = np.random.default_rng(23).random((30, 30, 30)) < 0.15  # a free border: one cell of offset clips nothing
    xa = np.argwhere(np.random.default_rng(24).random((32, 32, 32)) < 0.15)
    xb = np.argwhere(g) if max(abs(o) for o in offset) <= 1 else np.argwhere(np.random.default_rng(23).random((32, 32, 32)) < 0.15)
    out = assert_all(mv, xa, xb, 32, offset=offset, flags=(0,))
    clipped = out[E.UNION, 0]["clipped"]
    if max(abs(o) for o in offset) <= 1:
        assert clipped == 0
    elif max(abs(o) for o in offset) >= 32:
        assert clipped == len(xb) and len(out[E.INTERSECTION, 0]["xyz"]) == 0  # (assert_all saw the in-place intersection refused)
    else:
        assert 0 < clipped < len(xb)


def test_one_face_layer_is_clipped(mv):
    xb = full(8)
    xa = np.argwhere(np.random.default_rng(5).random((8, 8, 8)) < 0.5)
    for offset in ((1, 0, 0), (0, 0, -1)):
        out = assert_all(mv, xa, xb, 8, offset=offset, flags=(0,))
        assert out[E.UNION, 0]["clipped"] == 64 and len(out[E.UNION, 0]["xyz"]) == len(xa) + 448 - out[E.UNION, 0]["overlap"]


def test_nothing_wraps_at_the_largest_grid(mv):
    R, y, z = 1 << 21, 5, 9
    xyz = [(0, y, z), (R - 1, y, z), (0, y + 1, z), (R - 1, R - 1, R - 1), (R - 2, R - 2, R - 1), (R - 1, 0, 0), (0, 1, 0), (0, 0, 0)]
    a = build(mv, xyz, R)
    assert a.info().levels == 21
    for offset in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, 0, -1), (1, 1, 1), (-1, -1, -1), (R - 1, 0, 0), (-R, 0, 0), (R, R, R), (0, 1 - R, 0)):
        for op in E.OPS:
            want = assert_listing(a, a, op, offset)
            assert (want["xyz"].astype(np.int64) < R).all()
        moved = np.array(xyz, np.int64) + offset
        assert assert_listing(a, a, E.UNION, offset)["clipped"] == int((~((moved >= 0) & (moved < R)).all(1)).sum())
    assert_in_place(mv, build(mv, xyz, R), a, E.UNION, (1, 0, 0))
    assert_in_place(mv, build(mv, xyz, R), a, E.DIFFERENCE, (0, -1, 0))
    assert_in_place(mv, build(mv, xyz, R), a, E.XOR, (-1, -1, -1), E.ATTRIB_B)
    # a small brush into the far corner of the largest grid, and the largest grid into a small one
    brush = build(mv, full(2), 2, seed=9)
    want = assert_listing(a, brush, E.UNION, (R - 2, R - 2, R - 2))
    assert want["clipped"] == 0 and want["overlap"] == 2
    want = assert_listing(a, brush, E.UNION, (R - 1, R - 1, R - 1))
    assert want["clipped"] == 7 and want["overlap"] == 1
    want = assert_listing(brush, a, E.UNION)  # only (0, 0, 0) and (0, 1, 0) of a lie in the brush's grid
    assert want["clipped"] == len(xyz) - 2 and want["overlap"] == 2
    assert assert_listing(brush, a, E.INTERSECTION, (1 - R, 1 - R, 1 - R))["overlap"] == 1


# ---- grids of different size --------------------------------------------------------------------------------------------------------------------------------------
def test_a_brush_stamped_into_a_larger_grid(mv):
    xa = np.argwhere(np.random.default_rng(41).random((64, 64, 64)) < 0.05)
    brush = np.argwhere(np.random.default_rng(42).random((4, 4, 4)) < 0.7)
    out = assert_all(mv, xa, brush, 64, offset=(29, 30, 31), res_b=4)
    assert out[E.UNION, 0]["clipped"] == 0
    assert_all(mv, xa, brush, 64, res_b=4, flags=(0,))  # zero offset: b's codes as they are
    out = assert_all(mv, xa, brush, 64, offset=(62, -1, 10), res_b=4, flags=(0,))
    assert 0 < out[E.UNION, 0]["clipped"] < len(brush)


def test_b_on_a_larger_grid_is_clipped(mv):
    xa = np.argwhere(np.random.default_rng(43).random((8, 8, 8)) < 0.4)
    xb = np.argwhere(np.random.default_rng(44).random((32, 32, 32)) < 0.3)
    out = assert_all(mv, xa, xb, 8, res_b=32)  # zero offset, but codes beyond a's grid
    inside = (xb < 8).all(1).sum()
    assert out[E.UNION, 0]["clipped"] == len(xb) - inside > 0
    assert_all(mv, xa, xb, 8, offset=(-20, -3, 2), res_b=32, flags=(0,))


# ---- a == b ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", E.OPS)
@pytest.mark.parametrize("flags", [0, E.ATTRIB_B])
def test_a_combined_with_itself_shifted(mv, op, flags):
    xyz = np.argwhere(np.random.default_rng(51).random((16, 16, 16)) < 0.3)
    a = build(mv, xyz, 16)
    want = assert_listing(a, a, op, (1, 0, 0), flags)
    assert 0 < want["overlap"] < len(xyz)
    assert_in_place(mv, a, a, op, (1, 0, 0), flags)
    if op == E.UNION:  # the directional smear
        assert a.info().numberOfVoxels > len(xyz)


# ---- attributes -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_attrib_b_as_the_only_change(mv):
    xyz = np.argwhere(np.random.default_rng(61).random((16, 16, 16)) < 0.3)
    dark, glow = colours(len(xyz), 3, emission=False), colours(len(xyz), 4, emission=True)
    sub = np.arange(len(xyz)) % 3 == 0
    for a_at, b_at, he in ((dark, glow, 1), (glow, dark, 0)):  # hasEmission recomputed both ways
        a, b = build(mv, xyz, 16, attribs=a_at), build(mv, xyz, 16, attribs=b_at)
        nodes, view = octree(a)[0], a.device_view()
        assert a.info().hasEmission == 1 - he
        assert_in_place(mv, a, b, E.UNION, None, E.ATTRIB_B)
        assert a.info().hasEmission == he and np.array_equal(octree(a)[0], nodes) and np.array_equal(a.read_voxels()[1], b.read_voxels()[1])
        assert (a.device_view().nodes, a.device_view().attrs) == (view.nodes, view.attrs)  # the arrays stay where they were: written in place
    # a subset of a as b: the intersection under the flag removes and recolours at once; the union recolours the subset only
    a, b = build(mv, xyz, 16, attribs=dark), build(mv, xyz[sub], 16, attribs=glow[sub])
    xa, a0 = a.read_voxels()
    in_b = np.isin(S.morton(xa), S.morton(xyz[sub]))
    assert_in_place(mv, a, b, E.UNION, None, E.ATTRIB_B)
    got = a.read_voxels()[1]
    assert np.array_equal(got[in_b], b.read_voxels()[1]) and np.array_equal(got[~in_b], a0[~in_b]) and not np.array_equal(got[in_b], a0[in_b])
    assert_in_place(mv, build(mv, xyz, 16, attribs=dark), b, E.INTERSECTION, None, E.ATTRIB_B)
    # no effect on difference and xor
    c = build(mv, np.argwhere(np.random.default_rng(62).random((16, 16, 16)) < 0.3), 16, seed=6)
    for op in (E.DIFFERENCE, E.XOR):
        plain, flagged = a.combine_voxels(c, op), a.combine_voxels(c, op, None, E.ATTRIB_B)
        assert all(np.array_equal(plain[k], flagged[k]) for k in ("xyz", "attribs", "source")) and len(plain["xyz"]) > 0
        assert_in_place(mv, twin_handle(mv, a), c, op, None, E.ATTRIB_B)


def twin_handle(mv, svo):
    x0, a0 = svo.read_voxels()
    return build(mv, x0, int(svo.info().gridRes), attribs=a0)


def with_raw_alpha(mv, svo):
    """the same octree with the alpha bytes 40 and 80 on every voxel: an upload keeps the caller's bytes, and so does its rebuild"""
    nodes, attrs, _ = svo.download()
    attrs[:, 3], attrs[:, 7] = 40, 80
    i = svo.info()
    raw = mv.IntersectorOctreeGPU()
    raw.upload(nodes, attrs, LOWER, DPS, int(i.gridRes), i.hasEmission, embeddedMask=bool(i.embeddedMask))
    raw.rebuild()
    assert (raw.read_voxels()[1][:, [3, 7]] == (40, 80)).all()
    return raw


def test_alpha_bytes_of_b_arrive_as_255(mv):
    """b after fill_enclosed with a host attribute whose alpha bytes are 40 and 80 (the fill is an edit and stores them as 255 itself), and the same octree as a
    rebuilt upload, which does carry 40 and 80: a voxel taken from b has 255 in both, a voxel of a keeps whatever a holds."""
    g = np.zeros((16, 16, 16), bool)
    g[3:12, 3:12, 3:12] = True
    g[5:10, 5:10, 5:10] = False
    filled = build(mv, np.argwhere(g), 16, seed=7)
    assert filled.fill_enclosed(np.array([10, 20, 30, 40, 50, 60, 70, 80], np.uint8)) == 125
    raw = with_raw_alpha(mv, filled)
    cells = [(6, 6, 6), (0, 0, 0)]  # one in the filled cavity, one outside
    a = build(mv, cells, 16)
    for b in (filled, raw):
        for op, flags in ((E.UNION, 0), (E.UNION, E.ATTRIB_B), (E.XOR, 0), (E.INTERSECTION, E.ATTRIB_B)):
            want = assert_listing(a, b, op, None, flags)
            from_b = (want["source"] == 2) | ((want["source"] == 3) & bool(flags))
            assert from_b.sum() >= 1 and (want["attribs"][from_b][:, [3, 7]] == 255).all()
            got = assert_in_place(mv, build(mv, cells, 16), b, op, None, flags).read_voxels()[1]
            assert (got[:, [3, 7]] == 255).all()
    # ... and as a the raw bytes stay verbatim, in the listing and in place (where no edit could have written them)
    want = assert_listing(raw, a, E.UNION)
    n = raw.info().numberOfVoxels
    assert ((want["attribs"][:, [3, 7]] == (40, 80)).all(1)).sum() == n and len(want["xyz"]) == n + 1
    assert_in_place(mv, raw, a, E.UNION)
    assert ((raw.read_voxels()[1][:, [3, 7]] == (40, 80)).all(1)).sum() == n
    assert_in_place(mv, raw, a, E.DIFFERENCE, (1, 0, 0))
    assert ((raw.read_voxels()[1][:, [3, 7]] == (40, 80)).all(1)).sum() == n - 1  # (7, 6, 6), a filled cell, went


# ---- every flavour, every way a handle comes to its codes ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed():
    return S.sorted_voxels(specks_and_block([(1, 1, 1), (10, 10, 1)]))


@pytest.mark.parametrize("flags_a", [0, 1, 2, 3])
@pytest.mark.parametrize("flags_b", [0, 1, 2, 3])
def test_every_flavour(mv, mixed, flags_a, flags_b):
    xb = np.argwhere(np.random.default_rng(78).random((32, 32, 32)) < 0.05)
    b = build(mv, xb, 32, flags_b, seed=3)
    a = build(mv, mixed, 32, flags_a)
    assert flags_a != 3 or a.info().flavour == 2  # the tree flavour
    flavour = a.info().flavour
    a.set_emission_scale(2.5)
    for op, off, f in ((E.UNION, (2, 0, -1), 0), (E.DIFFERENCE, None, 0), (E.XOR, (0, 3, 0), E.ATTRIB_B), (E.INTERSECTION, None, E.ATTRIB_B)):
        assert_listing(a, b, op, off, f)
        assert_in_place(mv, a, b, op, off, f, flags_a)
        assert a.info().flavour == flavour and a.info().emissionScale == 2.5


def test_after_an_edit_a_fill_a_closing_a_pruning_and_a_rebuild(mv):
    g = np.zeros((16, 16, 16), bool)
    g[4:11, 4:11, 4:11] = True
    g[5:10, 5:10, 5:10] = False
    stamp = build(mv, np.argwhere(np.random.default_rng(81).random((16, 16, 16)) < 0.1), 16, seed=8)
    svo = build(mv, np.argwhere(g), 16)
    svo.edit_voxels(np.array([(7, 7, 7), (1, 1, 1), (13, 1, 1), (14, 2, 2)], np.uint32), colours(4, 8))
    svo.edit_voxels(np.array([(4, 4, 4)], np.uint32), None, np.full(1, REMOVE, np.uint8))
    assert_listing(svo, stamp, E.XOR, (1, 0, 0))
    assert_in_place(mv, svo, stamp, E.UNION, (1, 0, 0))
    assert svo.fill_enclosed() > 0
    assert_listing(svo, stamp, E.DIFFERENCE)
    assert_in_place(mv, svo, stamp, E.DIFFERENCE)
    svo.close(1, 1)
    assert_in_place(mv, svo, stamp, E.XOR, (0, -2, 0), E.ATTRIB_B)
    svo.keep_components(1, keep_largest=1)
    assert_listing(stamp, svo, E.INTERSECTION, (0, 2, 0), E.ATTRIB_B)
    assert_in_place(mv, svo, stamp, E.UNION, None, E.ATTRIB_B)
    # an upload keeps no codes, as a or as b; after rebuild() it has them
    nodes, attrs, _ = svo.download()
    i = svo.info()
    up = mv.IntersectorOctreeGPU()
    up.upload(nodes, attrs, LOWER, DPS, 16, i.hasEmission, embeddedMask=bool(i.embeddedMask))
    for call in (lambda: up.combine_voxels_device(stamp, E.UNION), lambda: stamp.combine_voxels_device(up, E.UNION), lambda: up.combine(stamp, E.UNION), lambda: stamp.combine(up, E.UNION)):
        with pytest.raises(mv.MvrtError, match="keeps no Morton codes"):
            call()
    up.rebuild()
    assert_listing(up, stamp, E.XOR, (1, 1, 1))
    assert_listing(stamp, up, E.DIFFERENCE, (-1, 0, 0))
    assert_in_place(mv, up, stamp, E.DIFFERENCE, (1, 1, 1))


def bunny(mv, res):
    tris = bunny_tris()
    v = tris.reshape(-1, 3)
    lo = v.min(0)
    dps = np.float32((v.max(0) - lo).max() / np.float32(res))
    svo = mv.IntersectorOctreeGPU()
    svo.build(v, None, None, None, lo, dps, res)
    return svo, lo, dps


def test_bunny_minus_itself_shifted(mv):
    svo, _, _ = bunny(mv, 64)
    n = svo.info().numberOfVoxels
    want = assert_listing(svo, svo, E.DIFFERENCE, (3, 0, 0))
    assert 0 < len(want["xyz"]) < n and want["overlap"] > 0
    x0, a0 = svo.read_voxels()
    added, removed, clipped = svo.combine(svo, E.DIFFERENCE, (3, 0, 0))
    assert (added, removed) == (0, want["overlap"]) and clipped == want["clipped"]
    assert same(svo.read_voxels(), (want["xyz"], want["attribs"]))


def test_through_the_path_tracers_intersector_with_steps_in_flight(mv):
    """The same two steps around the call and around the edit it stands for: the step issued before finishes first on the old octree, the frame buffer is not
    cleared, and the second step renders the new set and accumulates on it."""
    base, lo, dps = bunny(mv, 64)
    res, w, h = 64, 64, 36
    rgba, hw, hh = mv.read_rgbe_file(os.path.join(GOLDEN, "monks_forest_s.hdr"))
    cam = probe_camera(lo, dps, res, focus=9.0, lens_r=0.05)
    x0, a0 = base.read_voxels()
    block, offset = base, (3, 0, 0)  # the model against itself, shifted
    ex, eat, eops, (added, removed) = E.edit_lists(x0, a0, x0, a0, res, E.XOR, offset)
    assert added > 0 and removed > 0
    frames = []
    for use_call in (True, False):
        pt = mv.PathTracer()
        pt.setup(None)
        pt.resizeFrameBufferIfNeeded(None, w, h)
        pt.loadHDRIPixels(None, rgba, hw, hh, rgba, hw, hh)
        svo = pt.m_intersectorOctreeGPU
        svo.build_voxels(x0, a0, origin=lo, dps=dps, gridRes=res)
        pt.step(None, cam)
        if use_call:
            assert svo.combine(block, E.XOR, offset)[:2] == (added, removed)
        else:
            svo.edit_voxels(ex, eat, eops)
        assert svo.info().numberOfVoxels == len(x0) + added - removed
        pt.step(None, cam)
        assert pt.getSteps() == 2
        frames.append(pt.read_framebuffer()[: w * h].copy())
        pt.cleanUp()
    assert np.array_equal(frames[0].view(np.uint32), frames[1].view(np.uint32))
    single = mv.PathTracer()  # the second step alone gives another picture: the first one was not cleared away
    single.setup(None)
    single.resizeFrameBufferIfNeeded(None, w, h)
    single.loadHDRIPixels(None, rgba, hw, hh, rgba, hw, hh)
    single.m_intersectorOctreeGPU.build_voxels(x0, a0, origin=lo, dps=dps, gridRes=res)
    single.m_intersectorOctreeGPU.combine(block, E.XOR, offset)
    single.step(None, cam)
    assert not np.array_equal(single.read_framebuffer()[: w * h].view(np.uint32), frames[0].view(np.uint32))
    single.cleanUp()


# ---- the contract ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair(mv, mixed):
    return build(mv, mixed, 32), build(mv, np.argwhere(np.random.default_rng(91).random((32, 32, 32)) < 0.05), 32, seed=4)


def test_null_outputs_and_capacity(mv, pair):
    a, b = pair
    off = (1, 2, 3)
    want = assert_listing(a, b, E.UNION, off)
    n, counts = len(want["xyz"]), (len(want["xyz"]), want["overlap"], want["clipped"])
    assert n > 1000 and want["overlap"] > 0 and want["clipped"] > 0
    xyz, at, src = mv.DeviceArray((n, 3), np.uint32), mv.DeviceArray((n, 8), np.uint8), mv.DeviceArray(n, np.uint8)
    assert a.combine_voxels_device(b, E.UNION, off) == counts  # the sizing call: the capacity is not asked
    assert a.combine_voxels_device(b, E.UNION, off, 0, n, xyz) == counts and np.array_equal(xyz.to_host(), want["xyz"])
    assert a.combine_voxels_device(b, E.UNION, off, 0, n, None, at) == counts and np.array_equal(at.to_host(), want["attribs"])
    assert a.combine_voxels_device(b, E.UNION, off, 0, n, None, None, src) == counts and np.array_equal(src.to_host(), want["source"])
    lib = mv.lib()
    o = np.array(off, np.int32)
    assert lib.mvrt_svo_combine_voxels(a._h, b._h, E.UNION, o.ctypes.data, 0, 0, None, None, None, None, None, None, None) == 0  # even the counts may be NULL
    assert lib.mvrt_svo_combine_voxels(a._h, b._h, E.UNION, o.ctypes.data, 0, n, xyz.ptr, None, None, None, None, None, None) == 0
    one = build(mv, [(1, 1, 1), (3, 3, 3)], 4)
    o1 = np.array((1, 1, 1), np.int32)
    assert lib.mvrt_svo_combine(one._h, one._h, E.UNION, o1.ctypes.data, 0, None, None, None, None) == 0 and one.info().numberOfVoxels == 3  # (3, 3, 3) + 1 is clipped
    assert lib.mvrt_svo_combine(one._h, one._h, E.UNION, None, 0, None, None, None, None) == 0 and one.info().numberOfVoxels == 3  # a NULL offset is zero
    wide, host = filled(mv, (n + 5, 3), np.uint32)  # a larger capacity writes the count's worth
    assert a.combine_voxels_device(b, E.UNION, off, 0, n + 5, wide) == counts
    assert np.array_equal(wide.to_host()[:n], want["xyz"]) and np.array_equal(wide.to_host()[n:], host[n:])
    # one short: the counts are still returned and nothing is written
    (xyz, xyz_host), (at, at_host), (src, src_host) = filled(mv, (n, 3), np.uint32), filled(mv, (n, 8), np.uint8), filled(mv, n, np.uint8)
    nn, nov, ncl = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    assert lib.mvrt_svo_combine_voxels(a._h, b._h, E.UNION, o.ctypes.data, 0, n - 1, xyz.ptr, at.ptr, src.ptr, C.byref(nn), C.byref(nov), C.byref(ncl), None) != 0
    assert (nn.value, nov.value, ncl.value) == counts and b"capacity %d" % (n - 1) in lib.mvrt_last_error() and b"%d voxels" % n in lib.mvrt_last_error()
    for dev, host in ((xyz, xyz_host), (at, at_host), (src, src_host)):
        assert np.array_equal(dev.to_host(), host)
    with pytest.raises(mv.MvrtError, match="nothing was written"):
        a.combine_voxels_device(b, E.XOR, off, 0, 0, None, None, src)
    assert np.array_equal(src.to_host(), src_host)
    # an empty result is a success
    assert a.combine_voxels_device(b, E.INTERSECTION, (32, 0, 0), 0, 0, xyz, at, src) == (0, 0, b.info().numberOfVoxels)
    got = a.combine_voxels(b, E.INTERSECTION, (0, -32, 0))
    assert got["xyz"].shape == (0, 3) and got["attribs"].shape == (0, 8) and got["source"].shape == (0,)
    assert np.array_equal(xyz.to_host(), xyz_host)


def test_refusals_without_gpu_work(mv, pair):
    a, b = pair
    empty = mv.IntersectorOctreeGPU()
    nodes, attrs, _ = a.download()
    i = a.info()
    up = mv.IntersectorOctreeGPU()
    up.upload(nodes, attrs, LOWER, DPS, 32, i.hasEmission, embeddedMask=bool(i.embeddedMask))
    state = [(bytes(h.info()), octree(h)) for h in (a, b)]
    allocs = mv.allocation_state()[2]
    for h, text in ((empty, "no octree"), (up, "keeps no Morton codes")):
        for call in (lambda: h.combine_voxels_device(b, E.UNION), lambda: a.combine_voxels_device(h, E.UNION), lambda: h.combine(b, E.UNION), lambda: a.combine(h, E.UNION)):
            with pytest.raises(mv.MvrtError, match=text):
                call()
    for call in (a.combine_voxels_device, a.combine):
        for op in (-1, 4):
            with pytest.raises(mv.MvrtError, match="unknown op"):
                call(b, op)
        for flags in (2, 3, 0x80000000):
            with pytest.raises(mv.MvrtError, match="unknown flags"):
                call(b, E.UNION, None, flags)
        for off in ((2 ** 21 + 1, 0, 0), (0, -2 ** 21 - 1, 0), (0, 0, 2 ** 31 - 1), (-2 ** 31, 0, 0)):
            with pytest.raises(mv.MvrtError, match="outside"):
                call(b, E.UNION, off)
    assert mv.allocation_state()[2] == allocs  # on the host, before any GPU work
    assert a.combine_voxels_device(b, E.UNION, (2 ** 21, -2 ** 21, 0))[2] == b.info().numberOfVoxels  # the ends of the range are legal
    with pytest.raises(mv.MvrtError, match="would leave no voxel"):
        a.combine(b, E.INTERSECTION, (2 ** 21, 0, 0))
    for h, (info, before) in zip((a, b), state):
        assert bytes(h.info()) == info and same(octree(h), before)


def test_the_listing_modifies_neither_handle(mv, pair):
    a, b = pair
    state, held = [(bytes(h.info()), octree(h)) for h in (a, b)], mv.allocation_state()[:2]
    for op in E.OPS:
        assert_listing(a, b, op, (3, -2, 1), E.ATTRIB_B)
        assert_listing(a, b, op)
    for h, (info, before) in zip((a, b), state):
        assert bytes(h.info()) == info and same(octree(h), before)
    assert mv.allocation_state()[:2] == held  # the scratch is gone
