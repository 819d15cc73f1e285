"""The numpy model of the morphology calls (tests/morph_expected.py) without a GPU: against a brute force that visits every cell of the grid, the identities the
outside-is-occupied erosion was chosen for (duality, a closing contains the set, an opening lies in it, both idempotent), the holed shell that the fill alone
cannot classify, and the exact floor of a 26-voxel mean."""
import itertools

import numpy as np
import pytest

import fill_expected as F
import morph_expected as M
from surface_expected import morton
from voxel_sets import holed_shell


def random_set(rng, res, density):
    xyz = np.argwhere(rng.random((res, res, res)) < density)
    if len(xyz) == 0:
        xyz = np.array([[res // 2] * 3])
    return xyz.astype(np.uint32), rng.integers(0, 256, (len(xyz), 8), dtype=np.uint8)


def as_set(xyz):
    return {tuple(int(v) for v in p) for p in np.asarray(xyz).reshape(-1, 3)}


def brute_step(vox, res, element, dilate):
    """one step over every cell of the grid, straight from the definition; vox: {cell: 8 bytes}"""
    offs = [d for d in itertools.product((-1, 0, 1), repeat=3) if (sum(map(abs, d)) == 1 if element == M.FACES else d != (0, 0, 0))]
    out = {}
    for c in itertools.product(range(res), repeat=3):
        nb = [tuple(a + b for a, b in zip(c, d)) for d in offs]
        nb = [n for n in nb if all(0 <= v < res for v in n)]
        if dilate:
            if c in vox:
                out[c] = vox[c]
            else:
                src = [vox[n] for n in nb if n in vox]
                if src:
                    a = [sum(int(s[k]) for s in src) // len(src) for k in range(8)]
                    a[3] = a[7] = 255
                    out[c] = np.array(a, np.uint8)
        elif c in vox and all(n in vox for n in nb):
            out[c] = vox[c]
    return out


def brute(op, xyz, attribs, res, element, steps):
    vox = {tuple(int(v) for v in p): a for p, a in zip(xyz, attribs)}
    first = dict(vox)
    for half in {"dilate": "d", "erode": "e", "close": "de", "open": "ed"}[op]:
        for _ in range(steps):
            vox = brute_step(vox, res, element, half == "d")
    if op == "open":
        vox = {c: first[c] for c in vox}
    cells = sorted(vox, key=lambda c: int(morton(np.array([c]))[0]))
    return np.array(cells, np.uint32).reshape(-1, 3), np.array([vox[c] for c in cells], np.uint8).reshape(-1, 8)


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("element", [M.FACES, M.CUBE])
def test_model_against_brute_force(element, sparse):
    rng = np.random.default_rng(5)
    for res, density in ((2, 0.3), (4, 0.2), (8, 0.08), (8, 0.6)):
        xyz, at = random_set(rng, res, density)
        for op, steps in (("dilate", 1), ("dilate", 2), ("erode", 1), ("close", 1), ("close", 2), ("open", 1)):
            got, want = M.morph(op, xyz, at, res, element, steps, sparse), brute(op, xyz, at, res, element, steps)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (res, density, op, steps)
        one = brute("dilate", xyz, at, res, element, 1)
        new = ~np.isin(morton(one[0]), morton(xyz))
        cells = M.dilation_cells(xyz, at, res, element, sparse)
        assert np.array_equal(cells["xyz"], one[0][new]) and np.array_equal(cells["attribs"], one[1][new])
        have = as_set(xyz)
        offs = M.OFFSETS[element]
        assert list(cells["count"]) == [sum(tuple(int(a) + b for a, b in zip(c, d)) in have for d in offs) for c in cells["xyz"]]
        gone = ~np.isin(morton(M._sorted(xyz, at)[0]), morton(brute("erode", xyz, at, res, element, 1)[0]))
        assert np.array_equal(M.erosion_voxels(xyz, res, element, sparse), np.flatnonzero(gone))


@pytest.mark.parametrize("element", [M.FACES, M.CUBE])
@pytest.mark.parametrize("res", [2, 4, 8, 16])
def test_duality_extensivity_and_idempotence(res, element):
    rng = np.random.default_rng(res * 2 + element)
    grid = as_set(np.argwhere(np.ones((res,) * 3, bool)))
    for density in (0.1, 0.5, 0.9, 0.05, 0.3, 0.7):
        xyz, at = random_set(rng, res, density)
        a = as_set(xyz)
        rest = np.array(sorted(grid - a), np.uint32).reshape(-1, 3)
        for k in (1, 2, 3):
            eroded = as_set(M.morph("erode", xyz, at, res, element, k)[0])
            if len(rest):  # duality: E^k(A) = grid \ D^k(grid \ A)
                assert eroded == grid - as_set(M.morph("dilate", rest, None, res, element, k)[0]), (density, k)
            closed, opened = M.morph("close", xyz, at, res, element, k), M.morph("open", xyz, at, res, element, k)
            assert as_set(closed[0]) >= a >= as_set(opened[0])
            assert as_set(M.morph("close", closed[0], closed[1], res, element, k)[0]) == as_set(closed[0])
            if len(opened[0]):
                assert as_set(M.morph("open", opened[0], opened[1], res, element, k)[0]) == as_set(opened[0])
            # voxels of A keep their bytes through a closing, the voxels an opening leaves theirs
            index = {c: i for i, c in enumerate(map(tuple, xyz.astype(np.int64)))}
            for got in (closed, opened):
                for c, b in zip(map(tuple, got[0].astype(np.int64)), got[1]):
                    assert c not in index or np.array_equal(b, at[index[c]])


def test_holed_shell_needs_the_cube_closing():
    xyz = holed_shell().astype(np.uint32)
    at = np.tile(np.array([200, 100, 50, 255, 0, 0, 0, 255], np.uint8), (len(xyz), 1))
    assert len(F.enclosed(xyz, 16)["xyz"]) == 0  # one missing voxel makes the whole interior exterior
    cube = M.morph("close", xyz, at, 16, M.CUBE, 1)[0]
    assert as_set(cube) - as_set(xyz) == {(7, 7, 10)}  # exactly the hole
    cells = F.enclosed(cube, 16)
    assert len(cells["xyz"]) == 125 and cells["nRegions"] == 1
    faces = M.morph("close", xyz, at, 16, M.FACES, 1)[0]
    added = as_set(faces) - as_set(xyz)
    assert len(added) == 44 and (7, 7, 10) not in added  # concave corners, and the hole still open
    assert len(F.enclosed(faces, 16)["xyz"]) == 0


def test_mean_of_26_distinct_colours_is_floored():
    xyz = np.array([p for p in itertools.product(range(1, 4), repeat=3) if p != (2, 2, 2)], np.uint32)
    rng = np.random.default_rng(26)
    at = np.zeros((26, 8), np.uint8)
    at[:, :3] = rng.permutation(256)[:26, None] + np.array([0, 0, 0])
    at[:, 1] = rng.permutation(256)[:26]
    at[:, 4:7] = rng.integers(0, 256, (26, 3))
    at[:, 3], at[:, 7] = 7, 9  # the source alphas are not read
    cells = M.dilation_cells(xyz, at, 8, M.CUBE)
    i = int(np.flatnonzero((cells["xyz"] == 2).all(1))[0])
    assert cells["count"][i] == 26
    sums = at.astype(np.int64).sum(0)
    want = [sums[0] // 26, sums[1] // 26, sums[2] // 26, 255, sums[4] // 26, sums[5] // 26, sums[6] // 26, 255]
    assert list(cells["attribs"][i]) == want
    assert any(sums[k] % 26 for k in (0, 1, 2, 4, 5, 6))  # a floor that differs from rounding somewhere
    faces = M.dilation_cells(xyz, at, 8, M.FACES)
    j = int(np.flatnonzero((faces["xyz"] == 2).all(1))[0])
    assert faces["count"][j] == 6
