"""The model of the nearest-voxel query (tests/query_expected.py) without a GPU: against the model of the enclosed cells (nearest_expected.enclosed_nearest) and
against the model of the distance band (ball_expected.distance_cells with the largest radius) on the cells those list, for the sets their own tests use; then the
limit, the two-set summary and the transfer on shapes whose answer is known by hand."""
import numpy as np

import ball_expected as B
import nearest_expected as N
import query_expected as Q
from voxel_sets import cavities, colours, shell


def test_model_against_the_enclosed_cells_and_the_band():
    for xyz, res in cavities():
        at = colours(len(xyz))
        for listing in (N.enclosed_nearest(xyz, at, res), B.distance_cells(xyz, at, res, 1024)):
            assert len(listing["xyz"]) > 100
            got = Q.nearest_voxels(xyz, at, listing["xyz"])
            assert np.array_equal(got["dist2"], listing["dist2"].astype(np.uint64)) and np.array_equal(got["nearest"], listing["nearest"])
            assert np.array_equal(got["attribs"], listing["attribs"])
    cage = shell(1, 6)  # the ties of tests/test_nearest_cpu.py
    got = Q.nearest_voxels(cage, None, [(3, 3, 3), (2, 2, 2)])
    order = Q.sorted_set(cage)[0]
    assert got["dist2"].tolist() == [4, 1] and order[got["nearest"]].tolist() == [[3, 3, 1], [2, 2, 1]]


def test_points_outside_the_grid_the_limit_and_the_widths():
    xyz = np.array([(0, 0, 0), ((1 << 21) - 1,) * 3])
    m = 1 << 22
    got = Q.nearest_voxels(xyz, None, [(-m, -m, -m), (m, m, m), (m, -m, m), (5, 0, 0)])
    assert got["dist2"].dtype == np.uint64 and got["nearest"].dtype == np.uint32
    assert got["dist2"].tolist() == [3 << 44, 3 * (m - (1 << 21) + 1) ** 2, 2 * (m - (1 << 21) + 1) ** 2 + (m + (1 << 21) - 1) ** 2, 25] and got["nearest"].tolist() == [0, 1, 1, 0]
    far = Q.nearest_voxels(xyz[1:], None, [(-m, -m, -m)])["dist2"][0]
    assert (1 << 46) < far < (1 << 47)  # the largest d2 there is
    for limit, within in ((0, False), (24, False), (25, True), (26, True), (Q.NO_LIMIT, True)):
        got = Q.nearest_voxels(xyz, None, [(5, 0, 0)], limit)
        assert (got["dist2"].tolist(), got["nearest"].tolist()) == (([25], [0]) if within else ([Q.NO_LIMIT], [Q.NONE]))
        assert got["attribs"].tolist() == [[255, 255, 255, 255, 0, 0, 0, 255] if within else [0] * 8]


def test_two_sets_and_the_transfer_by_hand():
    a, b = np.array([(1, 1, 1), (4, 1, 1), (9, 1, 1)]), np.array([(1, 1, 1), (5, 1, 1)])
    r = Q.nearest_between(a, b)
    assert (r["dist2"].tolist(), r["nearest"].tolist()) == ([0, 1, 16], [0, 1, 1])
    assert (r["n"], r["maxDist2"], r["farthest"], r["zero"], r["beyond"]) == (3, 16, 2, 1, 0)
    r = Q.nearest_between(a, b, (0, 0, 0), 1)
    assert (r["maxDist2"], r["farthest"], r["beyond"]) == (1, 1, 1) and r["dist2"][2] == Q.NO_LIMIT
    r = Q.nearest_between(a, b, (4, 0, 0))  # b + o = (5, 1, 1), (9, 1, 1)
    assert r["dist2"].tolist() == [16, 1, 0] and r["farthest"] == 0
    assert Q.nearest_between(a, b, (0, 50, 0), 7)["farthest"] == Q.NONE
    da = np.array([[1, 2, 3, 4, 5, 6, 7, 8], [9, 9, 9, 9, 0, 0, 0, 0], [7, 7, 7, 255, 1, 1, 1, 255]], np.uint8)
    sa = np.array([[10, 20, 30, 40, 50, 60, 70, 80], [11, 21, 31, 41, 51, 61, 71, 81]], np.uint8)
    _, new, taken, changed = Q.transferred(a, da, b, sa, (0, 0, 0), 1, 1)
    assert taken.tolist() == [True, True, False] and changed == 2
    assert new.tolist() == [[10, 20, 30, 255, 5, 6, 7, 255], [11, 21, 31, 255, 0, 0, 0, 255], [7, 7, 7, 255, 1, 1, 1, 255]]
    _, new, _, changed = Q.transferred(a, da, a, da)  # from itself: only the alphas
    assert changed == 2 and np.array_equal(new, Q.alpha255(da))
