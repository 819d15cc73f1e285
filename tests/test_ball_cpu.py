"""The numpy model of the round offsets (tests/ball_expected.py) without a GPU, on random sets at 16^3: as SETS a ball of 1 and of 3 is one FACES and one CUBE step
of the morphology model, erosion is the dilation of the complement, a closing contains the set, an opening lies in it, both are idempotent, a ball of 2 is the
18-neighbourhood, a tie goes to the lowest vIndex, and the dense and the sparse form agree."""
import itertools

import numpy as np
import pytest

import ball_expected as B
import morph_expected as M
from surface_expected import morton

RES = 16


def random_set(seed, density, res=RES):
    rng = np.random.default_rng(seed)
    xyz = np.argwhere(rng.random((res, res, res)) < density)
    if len(xyz) == 0:
        xyz = np.array([[res // 2] * 3])
    return xyz.astype(np.uint32), rng.integers(0, 256, (len(xyz), 8), dtype=np.uint8)


def as_set(xyz):
    return {tuple(int(v) for v in p) for p in np.asarray(xyz).reshape(-1, 3)}


def complement(xyz, res=RES):
    s = as_set(xyz)
    return np.array([c for c in itertools.product(range(res), repeat=3) if c not in s], np.uint32).reshape(-1, 3)


CASES = [(seed, density) for seed, density in ((1, 0.02), (2, 0.2), (3, 0.6), (4, 0.9))]


@pytest.mark.parametrize("seed,density", CASES)
@pytest.mark.parametrize("rho,element", [(1, M.FACES), (3, M.CUBE)])
def test_ball_of_1_and_3_are_the_faces_and_the_cube_step_as_sets(seed, density, rho, element):
    xyz, at = random_set(seed, density)
    for op in ("dilate", "erode"):
        assert as_set(B.ball(op, xyz, at, RES, rho)[0]) == as_set(M.morph(op, xyz, at, RES, element, 1)[0])
    assert np.array_equal(B.distance_cells(xyz, at, RES, rho)["xyz"], M.dilation_cells(xyz, at, RES, element)["xyz"])
    assert np.array_equal(B.depth_voxels(xyz, RES, rho)["vIndex"], M.erosion_voxels(xyz, RES, element))


@pytest.mark.parametrize("seed,density", CASES)
@pytest.mark.parametrize("rho", [1, 2, 4, 5, 9, 14])
def test_erosion_is_the_dilation_of_the_complement(seed, density, rho):
    xyz, at = random_set(seed, density)
    rest = complement(xyz)
    if len(rest) == 0:
        return
    grown = as_set(B.ball("dilate", rest, None, RES, rho)[0])
    assert as_set(B.ball("erode", xyz, at, RES, rho)[0]) == set(itertools.product(range(RES), repeat=3)) - grown


@pytest.mark.parametrize("seed,density", CASES)
@pytest.mark.parametrize("rho", [1, 2, 5, 9])
def test_closing_contains_opening_lies_within_and_both_are_idempotent(seed, density, rho):
    xyz, at = random_set(seed, density)
    a = as_set(xyz)
    closed, cat = B.ball("close", xyz, at, RES, rho)
    assert a <= as_set(closed)
    again, aat = B.ball("close", closed, cat, RES, rho)
    assert np.array_equal(again, closed) and np.array_equal(aat, cat)
    opened, oat = B.ball("open", xyz, at, RES, rho)
    assert as_set(opened) <= a
    if len(opened):
        again, aat = B.ball("open", opened, oat, RES, rho)
        assert np.array_equal(again, opened) and np.array_equal(aat, oat)
        index = {int(c): i for i, c in enumerate(morton(xyz))}  # a pure removal: the bytes the voxel had
        assert np.array_equal(oat, at[[index[int(c)] for c in morton(opened)]])
    # cells of the set keep their bytes through a closing
    index = {int(c): i for i, c in enumerate(morton(closed))}
    assert np.array_equal(cat[[index[int(c)] for c in morton(xyz)]], at)


def test_ball_of_2_is_the_18_neighbourhood():
    got = B.distance_cells([[8, 8, 8]], None, RES, 2)
    want = {(8 + d[0], 8 + d[1], 8 + d[2]) for d in itertools.product((-1, 0, 1), repeat=3) if 0 < sum(map(abs, d)) <= 2}
    assert as_set(got["xyz"]) == want and len(want) == 18
    assert sorted(got["dist2"].tolist()) == [1] * 6 + [2] * 12


@pytest.mark.parametrize("sparse", [False, True])
def test_tie_goes_to_the_lowest_vindex(sparse):
    # two voxels two apart: the cell between them is equidistant; vIndex is the Morton rank: (5, 8, 8) before (7, 8, 8)
    xyz = np.array([[7, 8, 8], [5, 8, 8]], np.uint32)
    at = np.array([[10, 20, 30, 7, 1, 2, 3, 9], [200, 210, 220, 0, 4, 5, 6, 0]], np.uint8)
    got = B.distance_cells(xyz, at, RES, 1, sparse)
    i = [tuple(p) for p in got["xyz"].tolist()].index((6, 8, 8))
    assert got["dist2"][i] == 1 and got["nearest"][i] == 0 and got["attribs"][i].tolist() == [200, 210, 220, 255, 4, 5, 6, 255]
    # four voxels around a centre cell, each at distance 1: the lowest of the four
    xyz = np.array([[9, 8, 8], [8, 9, 8], [7, 8, 8], [8, 7, 8]], np.uint32)
    got = B.distance_cells(xyz, None, RES, 1, sparse)
    i = [tuple(p) for p in got["xyz"].tolist()].index((8, 8, 8))
    order = np.argsort(morton(xyz))
    assert got["nearest"][i] == 0 and tuple(xyz[order[0]]) == (8, 7, 8)
    # and the distance wins over the index: (6, 8, 8) lies next to vIndex 1 = (7, 8, 8), two cells from nobody else
    j = [tuple(p) for p in got["xyz"].tolist()].index((6, 8, 8))
    assert got["dist2"][j] == 1 and tuple(xyz[order[got["nearest"][j]]]) == (7, 8, 8)


@pytest.mark.parametrize("rho", [1, 2, 3, 4, 5, 8, 9, 14])
def test_dense_and_sparse_forms_agree_and_match_brute_force(rho):
    xyz, at = random_set(7, 0.03, 12)
    dense, sparse = B.distance_cells(xyz, at, 12, rho), B.distance_cells(xyz, at, 12, rho, sparse=True)
    for k in dense:
        assert np.array_equal(dense[k], sparse[k]), k
    dd, ds = B.depth_voxels(xyz, 12, rho), B.depth_voxels(xyz, 12, rho, sparse=True)
    assert np.array_equal(dd["vIndex"], ds["vIndex"]) and np.array_equal(dd["depth2"], ds["depth2"])
    # brute force over every cell of the grid, straight from the definition
    order = np.argsort(morton(xyz))
    v = xyz[order].astype(np.int64)
    want = {}
    for c in itertools.product(range(12), repeat=3):
        d2 = ((v - np.array(c)) ** 2).sum(1)
        if d2.min() > 0 and d2.min() <= rho:
            want[c] = (int(d2.min()), int(np.argmin(d2)))  # (argmin: the first, that is the lowest vIndex)
    got = {tuple(p): (int(d), int(n)) for p, d, n in zip(dense["xyz"].tolist(), dense["dist2"], dense["nearest"])}
    assert got == want


def test_border_and_full_grid():
    # a corner voxel of a 2^3 grid: clipped to the grid; the full grid: nothing to add, nothing to remove
    assert len(B.distance_cells([[0, 0, 0]], None, 2, 1)["xyz"]) == 3 and len(B.distance_cells([[0, 0, 0]], None, 2, 2)["xyz"]) == 6
    assert len(B.distance_cells([[0, 0, 0]], None, 2, 3)["xyz"]) == 7
    full = np.array(list(itertools.product(range(2), repeat=3)), np.uint32)
    assert len(B.distance_cells(full, None, 2, 3)["xyz"]) == 0 and len(B.depth_voxels(full, 2, 3)["vIndex"]) == 0
    # the far corner of the largest grid in the sparse form: no wrap in the 21 bits per axis
    m = (1 << 21) - 1
    got = B.distance_cells([[m, m, m]], None, 1 << 21, 4, sparse=True)
    # the octant of B(4) without its centre: three of length 1, three of 2, one of 3 and three of 4
    assert len(got["xyz"]) == 10 and got["xyz"].min() >= m - 2 and got["xyz"].max() == m
