"""Affine resampling of a voxel set on the GPU (mvrt_svo_resample_voxels / mvrt_svo_resample) against the numpy model of tests/resample_expected.py, bit for bit:
the listing array by array (xyz, attribs, source, the count, the sizing call), the build through a twin handle that build_voxels made from the model's list.  On the
smallest inputs that can break each mechanism -- gridRes 2 with one voxel under every signed permutation, a list of one, the workgroup seam at 255 / 256 / 257
entries of a frontier and of the result, a lone voxel that one destination centre maps into under a skew turn (where pruning would lose a thin hit), thin lines and
planes, anisotropic, sheared, singular and out-of-grid maps, grids of different size in both directions, the corners of the 2^21 grid, every flavour, edited /
filled / closed / rebuilt sources, an upload, dst == src, steps in flight, the bunny -- and the contract of the calls.  Grids up to 64^3 (128^3 for the bunny) are
checked against the dense form of the model, which evaluates the rule on every cell; larger ones against closed forms and the sparse form."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import combine_expected as CE
import resample_expected as E
import surface_expected as S
from common import GOLDEN, bunny_tris, probe_camera
from fixtures import load
from voxel_sets import DPS, LOWER, assert_same_octree, build, colours, filled, octree, same, specks_and_block

pytestmark = pytest.mark.gpu

REMOVE = 0
TURN30 = E.rotation((1, 2, 3), 30.0)


@pytest.fixture(scope="module")
def mv():
    m = load()
    assert m.TRANSFORM_FRAC_BITS == E.F
    return m


def model(src, mt, rd):
    xs, at = src.read_voxels()
    rs = int(src.info().gridRes)
    return (E.dense if rd <= 64 else E.sparse)(xs, at, rs, mt[0], mt[1], rd)


def assert_listing(mv, src, mt, rd=None, want=None, empty=False):
    """the listing against the model (or against `want`), array by array; returns the expected result"""
    rd = int(src.info().gridRes) if rd is None else rd
    want = model(src, mt, rd) if want is None else want
    xf = mv.CellTransform.make(*mt)
    got = src.resample_voxels(xf, rd)
    n = len(want["xyz"])
    print("Rs", src.info().gridRes, "Rd", rd, "|S|", src.info().numberOfVoxels, "n", len(got["xyz"]), "model", n, "frontier", mv.resample_stats()["frontier"])
    assert (n == 0) == empty  # a named case that is not called empty is not empty
    assert src.resample_voxels_device(xf, rd) == n  # the sizing call
    assert got["xyz"].dtype == np.uint32 and got["xyz"].shape == (n, 3) and np.array_equal(got["xyz"], want["xyz"])
    assert got["attribs"].dtype == np.uint8 and got["attribs"].shape == (n, 8) and np.array_equal(got["attribs"], want["attribs"])
    assert got["source"].dtype == np.uint32 and got["source"].shape == (n,) and np.array_equal(got["source"], want["source"])
    stats = mv.resample_stats()
    assert stats["levels"] == rd.bit_length() - 1 and (stats["frontier"][-1] == n or n == 0)
    return want


def assert_resampled(mv, src, mt, rd=None, flags=0, dst=None, want=None, origin=(0.5, -1.0, 2.0), dps=0.25):
    """src.resample into dst (None: a fresh handle) leaves the octree build_voxels builds from the model's list; src stays as it was when it is not dst"""
    rd = int(src.info().gridRes) if rd is None else rd
    want = model(src, mt, rd) if want is None else want
    assert len(want["xyz"]) > 0
    n_src = src.info().numberOfVoxels
    before, info = octree(src), bytes(src.info())
    dst = mv.IntersectorOctreeGPU() if dst is None else dst
    scale = dst.info().emissionScale  # the destination's own: the call does not touch it
    origin, dps = np.asarray(origin, np.float32), np.float32(dps)
    assert src.resample(mv.CellTransform.make(*mt), dst, origin, dps, rd, flags) is dst
    twin = build(mv, want["xyz"], rd, flags, want["attribs"], origin=origin, dps=dps)
    twin.set_emission_scale(scale)
    assert_same_octree(dst, twin, skip=("totalDumpedVoxels",))  # the resampling hands adoptSortedOnGrid the source's voxel count (csrc/api.hip), asserted below
    assert dst.info().totalDumpedVoxels == n_src and dst.info().hasEmission == int(want["attribs"][:, 4:7].any())
    if dst is not src:
        assert bytes(src.info()) == info and same(octree(src), before)
    return dst


def check(mv, xyz, rs, mt, rd=None, flags=0, src_flags=0, empty=False, seed=1):
    src = build(mv, xyz, rs, src_flags, seed=seed)
    want = assert_listing(mv, src, mt, rd, empty=empty)
    if not empty:
        assert_resampled(mv, src, mt, rd, flags, want=want)
    return want


def line(n, axis=0, at=(0, 1, 1)):
    xyz = np.tile(np.array(at, np.int64), (n, 1))
    xyz[:, axis] = np.arange(n)
    return xyz


# ---- the smallest inputs -----------------------------------------------------------------------------------------------------------------------------------------
def test_grid_res_2_one_voxel_under_every_signed_permutation(mv):
    for cell in ((1, 0, 1), (0, 0, 0)):
        want = check(mv, [cell], 2, E.identity())
        assert want["xyz"].tolist() == [list(cell)]
        perms = E.all_signed_permutations(2)
        assert len(perms) == 48
        src = build(mv, [cell], 2)
        for perm, flips, mt in perms:
            want = assert_listing(mv, src, mt)
            c = [0, 0, 0]
            for i in range(3):
                c[perm[i]] = 1 - cell[i] if flips[i] else cell[i]
            assert want["xyz"].tolist() == [c] and want["source"].tolist() == [0]
        assert_resampled(mv, src, perms[29][2])


def test_a_list_of_one_voxel(mv):
    for cell in ((0, 0, 0), (31, 31, 31), (13, 2, 30)):
        assert check(mv, [cell], 32, E.identity())["xyz"].tolist() == [list(cell)]
        want = check(mv, [cell], 32, E.signed_permutation((2, 0, 1), (1, 0, 1), 32), flags=3)
        assert want["xyz"].tolist() == [[cell[1], 31 - cell[2], 31 - cell[0]]]  # s = (31 - c_z, c_x, 31 - c_y)


def test_identity_on_a_random_set_is_read_voxels_with_alpha_255(mv):
    xyz = np.argwhere(np.random.default_rng(3).random((32, 32, 32)) < 0.2)
    src = build(mv, xyz, 32)
    want = assert_listing(mv, src, E.identity())
    x0, a0 = src.read_voxels()
    a0[:, [3, 7]] = 255
    assert len(x0) > 5000 and np.array_equal(want["xyz"], x0) and np.array_equal(want["attribs"], a0) and np.array_equal(want["source"], np.arange(len(x0)))
    assert_resampled(mv, src, E.identity(), want=want)


@pytest.mark.parametrize("offset", [(3, -2, 1), (0, 0, 31), (-32, 0, 0)])
def test_an_integer_translation_is_the_b_part_of_a_disjoint_union(mv, offset):
    """B' of mvrt_svo_combine_voxels: the set moved by whole cells and clipped; here the inverse map is s = c - offset"""
    xyz = np.argwhere(np.random.default_rng(4).random((32, 32, 32)) < 0.1)
    b = build(mv, xyz, 32)
    moved = xyz + np.array(offset)
    inside = ((moved >= 0) & (moved < 32)).all(1)
    free = np.setdiff1d(np.arange(32 ** 3, dtype=np.uint64), S.morton(moved[inside]))[:1]
    far = build(mv, S.decode(free), 32)  # one voxel the moved set does not meet
    got = far.combine_voxels(b, CE.UNION, offset)
    part = got["source"] == 2
    assert got["overlap"] == 0 and part.sum() == len(got["xyz"]) - 1
    want = assert_listing(mv, b, (E.identity()[0], -np.array(offset, np.int64) * 2 * E.ONE), empty=not inside.any())
    assert np.array_equal(got["xyz"][part], want["xyz"]) and np.array_equal(got["attribs"][part], want["attribs"])
    assert got["clipped"] == len(xyz) - len(want["xyz"]) == int((~inside).sum())  # the clipped count included


def test_magnification_2_and_4_in_blocks_and_sub_sampling(mv):
    xyz = np.argwhere(np.random.default_rng(5).random((16, 16, 16)) < 0.1)
    src = build(mv, xyz, 16)
    n = len(xyz)
    x0 = src.read_voxels()[0].astype(np.int64)
    for k, rd in ((1, 32), (2, 64)):
        mt = E.from_cells(np.eye(3) / (1 << k))
        want = assert_listing(mv, src, mt, rd)
        assert len(want["xyz"]) == n * 8 ** k and np.array_equal(want["xyz"].astype(np.int64) >> k, x0[want["source"]])
        assert np.array_equal(want["source"], np.repeat(np.arange(n, dtype=np.uint32), 8 ** k))  # whole blocks, in the order of the voxels
        assert_resampled(mv, src, mt, rd, want=want)
    # A = 2 I: s = 2 c + 1, the odd cells alone -- not the count rule of the coarsening
    mt = E.from_cells(np.eye(3) * 2)
    want = assert_listing(mv, src, mt, 8)
    odd = x0[(x0 % 2 == 1).all(1)]
    assert len(odd) > 0 and np.array_equal(want["xyz"], (odd >> 1)[np.argsort(S.morton(odd >> 1))])
    assert len(want["xyz"]) != len(src.coarse_voxels(1)["xyz"])
    assert_resampled(mv, src, mt, 8, want=want)


@pytest.mark.parametrize("rs,rd", [(8, 64), (64, 8), (32, 16), (4, 32), (2, 64), (64, 2)])
def test_grids_of_different_size(mv, rs, rd):
    xyz = np.argwhere(np.random.default_rng(rs + rd).random((rs, rs, rs)) < (1.0 if rd == 2 else 0.3))  # (8 samples of a thin set could all miss)
    check(mv, xyz, rs, E.about_centre(TURN30 * (rs / rd), rs, rd), rd)  # the same place in space on another lattice, turned
    check(mv, xyz, rs, E.identity(), rd, empty=False)  # cell for cell: the low corner of the larger grid


# ---- the workgroup seam ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [255, 256, 257])
def test_the_workgroup_seam_in_a_frontier_and_in_the_result(mv, n):
    """a line of n voxels from the grid's edge: the result has n entries; a line of 2 n: the frontier of the last-but-one level (nodes of two cells) has n"""
    R = 1024
    quarter = E.signed_permutation((1, 0, 2), (0, 1, 0), R)  # s = (c_y, R - 1 - c_x, c_z): a quarter turn about the grid centre, exact
    assert same(quarter, E.about_centre(E.rotation((0, 0, 1), -90.0), R, R))
    for count, frontier in ((n, None), (2 * n, n)):
        src = build(mv, line(count), R)
        x0, a0 = src.read_voxels()
        a0[:, [3, 7]] = 255
        want = assert_listing(mv, src, E.identity())
        assert np.array_equal(want["xyz"], x0) and np.array_equal(want["attribs"], a0) and len(x0) == count  # the closed form: the list itself
        assert frontier is None or mv.resample_stats()["frontier"][-2] == frontier
        turned = assert_listing(mv, src, quarter)
        c = np.stack([R - 1 - x0[:, 1].astype(np.int64), x0[:, 0], x0[:, 2]], 1)  # c_y = s_x, c_x = R - 1 - s_y
        o = np.argsort(S.morton(c))
        assert np.array_equal(turned["xyz"], c[o]) and np.array_equal(turned["source"], o.astype(np.uint32)) and np.array_equal(turned["attribs"], a0[o])
        assert frontier is None or mv.resample_stats()["frontier"][-2] == frontier  # a line along y from the edge y = 0
    assert_resampled(mv, src, quarter, want=turned)


# ---- thin hits under a skew turn ---------------------------------------------------------------------------------------------------------------------------------
def test_a_lone_voxel_that_exactly_one_centre_maps_into(mv):
    mt = E.about_centre(TURN30, 64, 64)
    cells = np.stack(np.meshgrid(*[np.arange(64, dtype=np.int64)] * 3, indexing="ij"), -1).reshape(-1, 3)
    s = E.point(mt[0], mt[1], cells)
    inside = ((s >= 0) & (s < 64)).all(1)
    codes, counts = np.unique(S.morton(s[inside]), return_counts=True)
    once = S.decode(codes[counts == 1])
    assert len(once) > 100  # a turn maps one or two centres into most cells; one into many
    for v in once[:: len(once) // 12]:
        want = check(mv, [v], 64, mt)
        assert len(want["xyz"]) == 1 and np.array_equal(E.point(mt[0], mt[1], want["xyz"])[0], v)
    none = np.setdiff1d(np.arange(64 ** 3, dtype=np.uint64)[:4096], codes)  # a cell no centre maps into, if the turn leaves one among the first codes
    for code in none[:2]:
        check(mv, S.decode(np.array([code], np.uint64)), 64, mt, empty=True)


def test_a_thin_diagonal_line_and_a_thin_plane_under_the_turn(mv):
    mt = E.about_centre(TURN30, 64, 64)
    k = np.arange(8, 56)
    diagonal = np.stack([k, k, k], 1)
    want = check(mv, diagonal, 64, mt)
    assert 30 < len(want["xyz"]) < 80
    plane = np.array([(x, y, 31) for x in range(6, 58) for y in range(6, 58)])
    want = check(mv, plane, 64, mt)
    assert 0.8 * len(plane) < len(want["xyz"]) < 1.2 * len(plane)


def test_anisotropic_sheared_and_general_maps(mv):
    xyz = np.argwhere(np.random.default_rng(7).random((32, 32, 32)) < 0.15)
    for A in (np.diag([4.0, 1.0, 0.1]), np.diag([0.1, 4.0, 1.0]) @ TURN30, np.array([[1, 0.5, 0], [0, 1, 0.25], [0, 0, 1.0]]), np.array([[0.3, -1.2, 0.4], [0.9, 0.2, -0.5], [1.1, 0.7, 0.8]])):
        want = check(mv, xyz, 32, E.about_centre(A, 32, 32))
        assert len(want["xyz"]) > 100


def test_singular_maps_and_maps_that_leave_the_grid(mv):
    cell = np.array([3, 5, 7])
    src = build(mv, [cell, (9, 9, 9)], 16)
    zero = np.zeros(9, np.int64)
    names = (zero, cell * 2 * E.ONE + E.HALF)  # every destination cell maps to the centre of that cell
    want = assert_listing(mv, src, names)
    assert len(want["xyz"]) == 4096 and (want["source"] == 0).all() and np.array_equal(want["xyz"], S.decode(np.arange(4096, dtype=np.uint64)))
    assert_resampled(mv, src, names, want=want)
    assert_resampled(mv, src, names, 32, flags=3)  # 32768 copies of one voxel
    before, info = octree(src), bytes(src.info())
    dst = build(mv, [(1, 1, 1)], 4)
    d_before, d_info = octree(dst), bytes(dst.info())
    misses = [(zero, np.array([3, 5, 6]) * 2 * E.ONE), (E.identity()[0], np.full(3, 64 * 2 * E.ONE)), (E.identity()[0], np.full(3, -64 * 2 * E.ONE)), (zero, np.array([-1, 0, 0]))]
    for mt in misses:  # an empty cell; the whole grid mapped outside the source, above and below
        assert_listing(mv, src, mt, empty=True)
        for d in (dst, src):
            with pytest.raises(mv.MvrtError, match="would leave no voxel"):
                src.resample(mv.CellTransform.make(*mt), d)
    assert bytes(src.info()) == info and same(octree(src), before) and bytes(dst.info()) == d_info and same(octree(dst), d_before)
    # rank 1 and rank 2
    xyz = np.argwhere(np.random.default_rng(8).random((16, 16, 16)) < 0.2)
    assert len(check(mv, xyz, 16, E.about_centre(np.outer([1, 0.5, -0.3], [0.4, 1, 0.2]), 16, 16))["xyz"]) > 0
    assert len(check(mv, xyz, 16, E.about_centre(np.diag([1.0, 1.0, 0.0]), 16, 16))["xyz"]) > 0  # a slice extruded along z


# ---- the largest grid --------------------------------------------------------------------------------------------------------------------------------------------
def test_the_corners_and_the_centre_of_the_largest_grid(mv):
    R = 1 << 21
    xyz = np.array([c for c in itertools.product((0, R - 1), repeat=3)] + [(R // 2, R // 2, R // 2)], np.int64)
    src = build(mv, xyz, R)
    assert src.info().levels == 21
    order = np.argsort(S.morton(xyz))
    at = src.read_voxels()[1]
    at[:, [3, 7]] = 255
    # a signed permutation plus a translation d: s_i = +-c_perm[i] ( + R - 1 ) + d_i; expected from the closed form, clipped to the grid
    for perm, flips, d in (((1, 2, 0), (1, 0, 1), (0, 0, 0)), ((2, 0, 1), (0, 1, 1), (1, -1, 0)), ((0, 1, 2), (0, 0, 0), (-1, -1, -1)), ((0, 2, 1), (1, 1, 1), (R - 1, 0, 0))):
        m, t = E.signed_permutation(perm, flips, R)
        t = t + np.array(d, np.int64) * 2 * E.ONE
        c = np.zeros_like(xyz)
        for i in range(3):
            u = xyz[:, i] - d[i]
            c[:, perm[i]] = R - 1 - u if flips[i] else u
        keep = ((c >= 0) & (c < R)).all(1)
        o = np.argsort(S.morton(c[keep]))
        want = {"xyz": c[keep][o].astype(np.uint32), "source": np.argsort(order)[keep][o].astype(np.uint32)}
        want["attribs"] = at[want["source"]]
        assert 0 < keep.sum() and same([E.sparse(xyz[order], at, R, m, t, R)[k] for k in ("xyz", "attribs", "source")], [want[k] for k in ("xyz", "attribs", "source")])
        assert_listing(mv, src, (m, t), want=want)
    assert_resampled(mv, src, (m, t), want=want, flags=1)
    # magnification 2 from 2^20: every voxel a 2x2x2 block at twice its coordinates
    half = 1 << 20
    small = np.array([c for c in itertools.product((0, half - 1), repeat=3)] + [(half // 2,) * 3], np.int64)
    src = build(mv, small, half)
    so = small[np.argsort(S.morton(small))]
    block = np.array(list(itertools.product((0, 1), repeat=3)))[:, ::-1]  # in Morton order: x fastest
    want = {"xyz": (2 * so[:, None, :] + block[None]).reshape(-1, 3).astype(np.uint32), "source": np.repeat(np.arange(9, dtype=np.uint32), 8)}
    want["attribs"] = src.read_voxels()[1][want["source"]]
    want["attribs"][:, [3, 7]] = 255
    mt = E.from_cells(np.eye(3) * 0.5)
    assert same([E.sparse(so, src.read_voxels()[1], half, mt[0], mt[1], R)[k] for k in ("xyz", "attribs", "source")], [want[k] for k in ("xyz", "attribs", "source")])
    assert_listing(mv, src, mt, R, want=want)
    assert_resampled(mv, src, mt, R, want=want)


# ---- every flavour, every way a handle comes to its codes ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed():
    return S.sorted_voxels(specks_and_block([(1, 1, 1), (10, 10, 1)]))


@pytest.mark.parametrize("src_flags", [0, 1, 2, 3])
@pytest.mark.parametrize("dst_flags", [0, 1, 2, 3])
def test_every_flavour(mv, mixed, src_flags, dst_flags):
    src = build(mv, mixed, 32, src_flags)
    assert src_flags != 3 or src.info().flavour == 2  # the tree flavour
    mt = E.about_centre(TURN30, 32, 32)
    want = assert_listing(mv, src, mt)
    dst = mv.IntersectorOctreeGPU()
    dst.set_emission_scale(2.5)
    assert_resampled(mv, src, mt, flags=dst_flags, dst=dst, want=want)
    assert dst.info().emissionScale == 2.5 and (dst_flags != 3 or dst.info().flavour == 2)
    with pytest.raises(mv.MvrtError, match="unsupported flags"):
        src.resample(mv.CellTransform.make(*mt), dst, flags=4)


def test_after_an_edit_a_fill_a_closing_and_a_rebuild_and_an_upload(mv):
    g = np.zeros((16, 16, 16), bool)
    g[4:11, 4:11, 4:11] = True
    g[5:10, 5:10, 5:10] = False
    mt = E.about_centre(TURN30 * 0.5, 16, 32)  # turned, onto a grid twice as fine
    svo = build(mv, np.argwhere(g), 16)
    svo.edit_voxels(np.array([(7, 7, 7), (1, 1, 1), (13, 1, 1), (14, 2, 2)], np.uint32), colours(4, 8))
    svo.edit_voxels(np.array([(4, 4, 4)], np.uint32), None, np.full(1, REMOVE, np.uint8))
    assert_resampled(mv, svo, mt, 32, want=assert_listing(mv, svo, mt, 32))
    assert svo.fill_enclosed(np.array([10, 20, 30, 40, 50, 60, 70, 80], np.uint8)) > 0
    assert_resampled(mv, svo, mt, 32, want=assert_listing(mv, svo, mt, 32))
    svo.close(1, 1)
    assert_resampled(mv, svo, mt, 32, want=assert_listing(mv, svo, mt, 32))
    # an upload keeps no codes; after rebuild() it has them, and alpha bytes the source carries arrive as 255
    nodes, attrs, _ = svo.download()
    attrs[:, 3], attrs[:, 7] = 40, 80
    i = svo.info()
    up = mv.IntersectorOctreeGPU()
    up.upload(nodes, attrs, LOWER, DPS, 16, i.hasEmission, embeddedMask=bool(i.embeddedMask))
    xf = mv.CellTransform.make(*mt)
    for call in (lambda: up.resample_voxels_device(xf, 32), lambda: up.resample_voxels(xf, 32), lambda: up.resample(xf, gridRes=32), lambda: up.resample(xf, svo, gridRes=32)):
        with pytest.raises(mv.MvrtError, match="keeps no Morton codes"):
            call()
    up.rebuild()
    assert (up.read_voxels()[1][:, [3, 7]] == (40, 80)).all()
    want = assert_listing(mv, up, mt, 32)
    assert (want["attribs"][:, [3, 7]] == 255).all()
    assert_resampled(mv, up, mt, 32, want=want)


def test_dst_is_src(mv, mixed):
    mt = E.about_centre(TURN30, 32, 32)
    for flags, rd in ((0, 32), (3, 64), (1, 16)):
        src = build(mv, mixed, 32, flags)
        src.set_emission_scale(1.5)
        m = mt if rd == 32 else E.about_centre(TURN30 * (32 / rd), 32, rd)
        want = model(src, m, rd)
        assert_resampled(mv, src, m, rd, flags, dst=src, want=want)
        assert src.info().emissionScale == 1.5 and src.info().gridRes == rd
    # the defaults of the Python wrapper: the source's own lattice, in place
    src = build(mv, mixed, 32)
    want, i = model(src, mt, 32), src.info()
    assert src.resample(mv.CellTransform.make(*mt)) is src
    j = src.info()
    assert np.array_equal(src.read_voxels()[0], want["xyz"]) and (j.lower[:], j.upper[:], j.dps, j.gridRes) == (i.lower[:], i.upper[:], i.dps, i.gridRes)


def test_resample_then_combine_is_the_rotated_stamp(mv, mixed):
    scene = build(mv, np.argwhere(np.random.default_rng(12).random((32, 32, 32)) < 0.05), 32, seed=3)
    stamp = build(mv, mixed, 32, seed=4)
    mt = E.about_centre(E.rotation((0, 1, 0), 45.0), 32, 32)
    turned = stamp.resample(mv.CellTransform.make(*mt), mv.IntersectorOctreeGPU())
    rs = model(stamp, mt, 32)
    xa, aa = scene.read_voxels()
    for op, off in ((CE.UNION, (2, 0, -1)), (CE.DIFFERENCE, None)):
        want = CE.combine(xa, aa, rs["xyz"], rs["attribs"], 32, op, off)
        got = scene.combine_voxels(turned, op, off)
        assert len(want["xyz"]) > 0 and all(np.array_equal(got[k], want[k]) for k in ("xyz", "attribs", "source"))
    scene.combine(turned, CE.UNION, (2, 0, -1))
    want = CE.combine(xa, aa, rs["xyz"], rs["attribs"], 32, CE.UNION, (2, 0, -1))
    assert same(scene.read_voxels(), (want["xyz"], want["attribs"]))


def bunny(mv, res):
    tris = bunny_tris()
    v = tris.reshape(-1, 3)
    lo = v.min(0)
    dps = np.float32((v.max(0) - lo).max() / np.float32(res))
    svo = mv.IntersectorOctreeGPU()
    svo.build(v, None, None, None, lo, dps, res)
    return svo, lo, dps


def test_bunny_at_128_under_the_turn_against_the_dense_model(mv):
    svo, lo, dps = bunny(mv, 128)
    xs, at = svo.read_voxels()
    mt = E.about_centre(TURN30, 128, 128)
    want = E.dense(xs, at, 128, mt[0], mt[1], 128)
    assert 0.5 * len(xs) < len(want["xyz"]) < 1.5 * len(xs)
    assert_listing(mv, svo, mt, want=want)
    assert_resampled(mv, svo, mt, want=want, origin=lo, dps=dps)
    # ... and through world space: the same turn about the middle of the bunny's box, made by cell_transform_from_world
    W = np.concatenate([TURN30, np.zeros((3, 1))], 1)
    centre = lo.astype(np.float64) + 64.0 * float(dps)
    W[:, 3] = centre - TURN30 @ centre
    xf = mv.cell_transform_from_world(W, lo, dps, lo, dps)
    m, t = xf.arrays()
    inv = E.about_centre(TURN30.T, 128, 128)  # the record holds the inverse of the world map
    assert np.abs(m - inv[0]).max() <= 64 and np.abs(t - inv[1]).max() <= 1 << 16  # lo and dps are float32: the lattice is known to about 2^-24 of its size
    assert_listing(mv, svo, (m, t), want=E.dense(xs, at, 128, m, t, 128))


def test_through_the_path_tracers_intersector_with_steps_in_flight(mv):
    """The same two steps around the call and around the voxel-list build it stands for: the step issued before finishes first on the old octree, the frame buffer
    is not cleared, and the second step renders the new set and accumulates on it."""
    base, lo, dps = bunny(mv, 64)
    res, w, h = 64, 64, 36
    rgba, hw, hh = mv.read_rgbe_file(os.path.join(GOLDEN, "monks_forest_s.hdr"))
    cam = probe_camera(lo, dps, res, focus=9.0, lens_r=0.05)
    x0, a0 = base.read_voxels()
    mt = E.about_centre(E.rotation((0, 1, 0), 90.0), res, res)
    want = E.dense(x0, a0, res, mt[0], mt[1], res)
    assert len(want["xyz"]) == len(x0) and not np.array_equal(want["xyz"], x0)
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
            base.resample(mv.CellTransform.make(*mt), svo)
        else:
            svo.build_voxels(want["xyz"], want["attribs"], origin=lo, dps=dps, gridRes=res)
        assert svo.info().numberOfVoxels == len(want["xyz"])
        pt.step(None, cam)
        assert pt.getSteps() == 2
        frames.append(pt.read_framebuffer()[: w * h].copy())
        pt.cleanUp()
    assert np.array_equal(frames[0].view(np.uint32), frames[1].view(np.uint32))


# ---- the contract ----------------------------------------------------------------------------------------------------------------------------------------------
def test_null_outputs_and_capacity(mv, mixed):
    src = build(mv, mixed, 32)
    mt = E.about_centre(TURN30, 32, 32)
    xf = mv.CellTransform.make(*mt)
    want = assert_listing(mv, src, mt)
    n = len(want["xyz"])
    assert n > 1000
    state, held = (bytes(src.info()), octree(src)), mv.allocation_state()[:2]
    xyz, at, so = mv.DeviceArray((n, 3), np.uint32), mv.DeviceArray((n, 8), np.uint8), mv.DeviceArray(n, np.uint32)
    assert src.resample_voxels_device(xf, 32, n, xyz) == n and np.array_equal(xyz.to_host(), want["xyz"])
    assert src.resample_voxels_device(xf, 32, n, None, at) == n and np.array_equal(at.to_host(), want["attribs"])
    assert src.resample_voxels_device(xf, 32, n, None, None, so) == n and np.array_equal(so.to_host(), want["source"])
    lib = mv.lib()
    assert lib.mvrt_svo_resample_voxels(src._h, C.byref(xf), 32, 0, None, None, None, None, None) == 0  # even the count may be NULL
    assert lib.mvrt_svo_resample_voxels(src._h, C.byref(xf), 32, n, xyz.ptr, None, None, None, None) == 0
    wide, host = filled(mv, (n + 5, 3), np.uint32)  # a larger capacity writes the count's worth
    assert src.resample_voxels_device(xf, 32, n + 5, wide) == n
    assert np.array_equal(wide.to_host()[:n], want["xyz"]) and np.array_equal(wide.to_host()[n:], host[n:])
    # one short: the count is still returned and nothing is written
    (xyz, xyz_host), (at, at_host), (so, so_host) = filled(mv, (n, 3), np.uint32), filled(mv, (n, 8), np.uint8), filled(mv, n, np.uint32)
    nn = C.c_uint64(0)
    assert lib.mvrt_svo_resample_voxels(src._h, C.byref(xf), 32, n - 1, xyz.ptr, at.ptr, so.ptr, C.byref(nn), None) != 0
    assert nn.value == n and b"capacity %d" % (n - 1) in lib.mvrt_last_error() and b"%d voxels" % n in lib.mvrt_last_error() and b"nothing was written" in lib.mvrt_last_error()
    for dev, host in ((xyz, xyz_host), (at, at_host), (so, so_host)):
        assert np.array_equal(dev.to_host(), host)
    # an empty result is a success and writes nothing
    out = (E.identity()[0], np.full(3, 64 * 2 * E.ONE))
    assert src.resample_voxels_device(mv.CellTransform.make(*out), 32, 0, xyz, at, so) == 0
    got = src.resample_voxels(mv.CellTransform.make(*out))
    assert got["xyz"].shape == (0, 3) and got["attribs"].shape == (0, 8) and got["source"].shape == (0,) and np.array_equal(xyz.to_host(), xyz_host)
    assert bytes(src.info()) == state[0] and same(octree(src), state[1]) and mv.allocation_state()[:2] == held  # src is never modified, the scratch is gone


def test_refusals_without_gpu_work(mv, mixed):
    src, dst = build(mv, mixed, 32), build(mv, [(1, 1, 1)], 4)
    state = [(bytes(h.info()), octree(h)) for h in (src, dst)]
    empty = mv.IntersectorOctreeGPU()
    allocs = mv.allocation_state()[2]
    ok = mv.CellTransform.make(*E.identity())

    def bad_record(**fields):
        x = mv.CellTransform.make(*E.identity())
        for k, v in fields.items():
            setattr(x, k, v)
        return x

    def entry(k, v, t=False):
        x = mv.CellTransform.make(*E.identity())
        (x.t if t else x.m)[k] = v
        return x

    cases = [(bad_record(structBytes=96), 32, "structBytes"), (bad_record(structBytes=0), 32, "structBytes"), (bad_record(reserved=1), 32, "reserved"),
             (entry(4, (1 << 30) + 1), 32, "out of range"), (entry(0, -(1 << 30) - 1), 32, "out of range"), (entry(2, (1 << 52) + 1, True), 32, "out of range"),
             (entry(0, -(1 << 63), True), 32, "out of range"), (ok, 3, "power of two"), (ok, 0, "power of two"), (ok, 1, "power of two"), (ok, -8, "power of two"),
             (ok, 1 << 22, "power of two")]
    for xf, rd, text in cases:
        for call in (lambda: src.resample_voxels_device(xf, rd), lambda: src.resample(xf, dst, gridRes=rd), lambda: src.resample(xf, gridRes=rd)):
            with pytest.raises(mv.MvrtError, match=text):
                call()
    with pytest.raises(mv.MvrtError, match="no octree"):
        empty.resample(ok, dst, origin=(0, 0, 0), dps=1.0, gridRes=4)
    lib = mv.lib()
    assert lib.mvrt_svo_resample_voxels(src._h, None, 32, 0, None, None, None, None, None) != 0 and b"null transform" in lib.mvrt_last_error()
    assert mv.allocation_state()[2] == allocs  # on the host, before any GPU work
    for h, (info, before) in zip((src, dst), state):
        assert bytes(h.info()) == info and same(octree(h), before)
    # the limits themselves are legal
    assert src.resample_voxels_device(entry(4, 1 << 30), 32) >= 0 and src.resample_voxels_device(entry(1, -(1 << 52), True), 32) >= 0
    assert dst.resample(ok, empty).info().numberOfVoxels == 1  # an empty handle as dst is the usual case
