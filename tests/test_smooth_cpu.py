"""The numpy model of the constrained surface nets (tests/smooth_expected.py) without a GPU: against figures computed on the CPU from the rule of
include/mvrt.h (vertex, face and degree counts, clamp counts, sums of |d|), and against properties the rule promises -- K = 0 is the plain weld bit for bit,
mirrored, axis-swapped and translated sets give mirrored, swapped and equal displacements, limit 0 moves nothing, limit <= 127 keeps every vertex apart, and the
position formula at gridRes 2^21 agrees with a float64 computation rounded at the same three places."""
import numpy as np
import pytest

import smooth_expected as M
import surface_expected as S

LOWER, DPS = np.array([-3.7, 0.1, 12.3], np.float32), np.float32(0.1)
PLATE = np.array([(x, y, 3) for x in range(1, 7) for y in range(1, 7)])
FIXTURES = {"voxel": (np.array([(1, 1, 1)]), 4), "ball16": (M.ball(16, 6.3), 16), "ball32": (M.ball(32, 13.7), 32), "plate": (PLATE, 8)}


def run(name, K, weights=(256, 256), limit=127):
    xyz, res = FIXTURES[name]
    return M.smooth(xyz, res, LOWER, DPS, K, weights, limit)


def degrees(w):
    n = np.array([bin(m).count("1") for m in w["neighbours"]])
    return [int((n == k).sum()) for k in (3, 4, 5, 6)]


def total(w):
    return int(np.abs(w["displacements"].astype(np.int64)).sum())


def test_one_voxel():
    w = run("voxel", 1, limit=128)
    assert len(w["corners"]) == 8 and len(w["indices"]) == 6 and degrees(w) == [8, 0, 0, 0]
    assert (np.abs(w["displacements"]) == 85).all() and w["clamped"] == 0
    w = run("voxel", 16, limit=96)
    assert (np.abs(w["displacements"]) == 96).all() and w["clamped"] == 360
    w = run("voxel", 64, limit=128)
    assert (np.abs(w["displacements"]) == 128).all() and w["clamped"] == 0
    assert len(np.unique(M.fixed_point(w), axis=0)) == 1 and (M.fixed_point(w) == 256 + 128).all()  # all eight at the cell centre: why limit <= 127


@pytest.mark.parametrize("name,counts,deg,cases", [
    ("ball16", (722, 720), [152, 450, 96, 24], [((4, (256, 256), 127), (192, 119976, None)), ((5, (128, -136), 127), (0, 60912, 64))]),
    ("ball32", (3554, 3552), [1008, 1674, 744, 128], [((4, (256, 256), 127), (576, 585216, None)), ((7, (128, -136), 64), (1848, 336798, None))]),
    ("plate", (98, 96), [8, 90, 0, 0], [((8, (256, 256), 127), (352, 21916, None))]),
])
def test_pins(name, counts, deg, cases):
    for (K, weights, limit), (clamped, sum_abs, max_abs) in cases:
        w = run(name, K, weights, limit)
        assert (len(w["corners"]), len(w["indices"])) == counts and degrees(w) == deg
        assert (w["clamped"], total(w)) == (clamped, sum_abs)
        if max_abs is not None:
            assert int(np.abs(w["displacements"]).max()) == max_abs


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_no_iteration_is_the_weld(name):
    xyz, res = FIXTURES[name]
    w = run(name, 0)
    want = S.surface(xyz, res, LOWER, DPS)
    assert np.array_equal(w["vertices"].view(np.uint32), want["vertices"].view(np.uint32)) and np.array_equal(w["indices"], want["indices"])
    assert np.array_equal(w["faceVoxel"], want["faceVoxel"]) and np.array_equal(w["faceDir"], want["faceDir"])
    assert not w["displacements"].any() and w["clamped"] == 0


def by_corner(w):
    """{corner: displacement}"""
    return {tuple(c): tuple(d) for c, d in zip(w["corners"].tolist(), w["displacements"].tolist())}


@pytest.mark.parametrize("weights,K", [((256, 256), 4), ((128, -136), 5)])
def test_mirror_swap_and_translation(weights, K):
    rng = np.random.default_rng(3)
    xyz = np.concatenate([M.ball(12, 4.4) + (1, 2, 0), np.argwhere(rng.random((12, 12, 12)) < 0.05)])
    res = 16
    base = by_corner(M.smooth(xyz, res, LOWER, DPS, K, weights, 127))
    mirrored = xyz.copy()
    mirrored[:, 0] = res - 1 - mirrored[:, 0]
    got = by_corner(M.smooth(mirrored, res, LOWER, DPS, K, weights, 127))
    assert got == {(res - c[0], c[1], c[2]): (-d[0], d[1], d[2]) for c, d in base.items()}
    got = by_corner(M.smooth(xyz[:, [0, 2, 1]], res, LOWER, DPS, K, weights, 127))
    assert got == {(c[0], c[2], c[1]): (d[0], d[2], d[1]) for c, d in base.items()}
    got = by_corner(M.smooth(xyz + (3, 1, 2), res, LOWER, DPS, K, weights, 127))
    assert got == {(c[0] + 3, c[1] + 1, c[2] + 2): d for c, d in base.items()}


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_limits(name):
    assert not run(name, 6, limit=0)["displacements"].any()
    for weights, limit, K in (((256, 256), 127, 4), ((256, 256), 127, 64), ((128, -136), 127, 9), ((256, -256), 100, 16)):
        w = run(name, K, weights, limit)
        assert np.abs(w["displacements"]).max() <= limit
        assert len(np.unique(M.fixed_point(w), axis=0)) == len(w["corners"])  # no two vertices meet


def test_positions_at_the_largest_grid():
    """q up to 2^29 + 128 rounds once in the conversion; float64 holds every intermediate exactly until it is rounded at the same three places"""
    R = 1 << 21
    rng = np.random.default_rng(7)
    c = np.concatenate([rng.integers(0, R + 1, size=(4000, 3)), [(0, 0, 0), (R, R, R), (R - 1, 1, R), (1, R - 1, 0)]]).astype(np.int64)
    d = rng.integers(-128, 129, size=c.shape)
    d[-4:] = [(128, -128, 0), (-128, 128, -1), (127, -127, 128), (-128, 128, 1)]
    got = M.positions(c, d, LOWER, DPS)
    q = (256 * c + d).astype(np.float64)
    t = (q.astype(np.float32).astype(np.float64) * 0.00390625).astype(np.float32)  # the conversion rounds, the scaling is exact
    assert np.array_equal(t.astype(np.float64), q.astype(np.float32).astype(np.float64) / 256.0)
    prod = (t.astype(np.float64) * np.float64(DPS)).astype(np.float32)
    want = (LOWER.astype(np.float64) + prod.astype(np.float64)).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    zero = M.positions(c, np.zeros_like(d), LOWER, DPS)
    assert np.array_equal(zero.view(np.uint32), S.positions(c, LOWER, DPS).view(np.uint32))  # d = 0: the bits of the plain mesh


def test_a_negative_weight_moves_border_corners_outwards():
    """the ranges allow a negative even weight: the corner (0, 0, 0) of a voxel on the grid border then leaves the grid, q = 256 c + d is negative there and
    the position lies below `lower`, by the same three-step formula"""
    w = M.smooth([(0, 0, 0)], 2, LOWER, DPS, 4, (-256, -256), 127)
    at = {tuple(c): tuple(d) for c, d in zip(w["corners"].tolist(), w["displacements"].tolist())}
    assert at[(0, 0, 0)] == (-127, -127, -127) and at[(1, 1, 1)] == (127, 127, 127)
    q = M.fixed_point(w)
    assert q.min() == -127 and len(np.unique(q, axis=0)) == 8
    t = (q.astype(np.float32).astype(np.float64) * 0.00390625).astype(np.float32)
    want = (LOWER.astype(np.float64) + (t.astype(np.float64) * np.float64(DPS)).astype(np.float32).astype(np.float64)).astype(np.float32)
    assert np.array_equal(w["vertices"].view(np.uint32), want.view(np.uint32)) and (w["vertices"][0] < LOWER).all()
