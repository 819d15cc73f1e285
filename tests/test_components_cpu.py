"""The model of the connected components (tests/components_expected.py) without a GPU: against hand-written answers for the smallest cases, against
scipy.ndimage.label (where scipy is installed) after renumbering by first appearance, the sparse form against the searchsorted form, and the selection rule."""
import numpy as np
import pytest

import components_expected as K
from surface_expected import morton


def first_appearance(raw):
    """any labelling -> the canonical numbering: 0, 1, ... in order of first appearance"""
    _, first, inverse = np.unique(raw, return_index=True, return_inverse=True)
    return np.argsort(np.argsort(first))[inverse]


def checkerboard(res):
    return np.argwhere(np.indices((res,) * 3).sum(0) % 2 == 0)


def test_tiny_cases_by_hand():
    c = K.components([(1, 0, 1)], 2, K.CUBE)
    assert c["label"].tolist() == [0] and c["size"].tolist() == [1] and c["first"].tolist() == [0] and c["box"].tolist() == [[1, 0, 1, 1, 0, 1]]
    full = np.argwhere(np.ones((2, 2, 2), bool))
    for e in (K.FACES, K.CUBE):
        c = K.components(full, 2, e)
        assert c["label"].tolist() == [0] * 8 and c["size"].tolist() == [8] and c["box"].tolist() == [[0, 0, 0, 1, 1, 1]]
    for other in ((1, 1, 0), (1, 1, 1)):  # an edge and a corner neighbour: two components under FACES, one under CUBE
        c = K.components([(0, 0, 0), other], 2, K.FACES)
        assert c["label"].tolist() == [0, 1] and c["size"].tolist() == [1, 1] and c["first"].tolist() == [0, 1]
        assert c["box"].tolist() == [[0, 0, 0, 0, 0, 0], list(other) * 2]
        c = K.components([other, (0, 0, 0)], 2, K.CUBE)  # (the order of the input does not matter)
        assert c["label"].tolist() == [0, 0] and c["size"].tolist() == [2] and c["first"].tolist() == [0] and c["box"].tolist() == [[0, 0, 0] + list(other)]


def test_seam_and_labels_in_morton_order():
    # across the top octant seam the codes are far apart; the voxel between them in Morton order is a component of its own and gets label 1
    c = K.components([(7, 3, 3), (8, 3, 3), (7, 7, 7)], 16, K.FACES)
    assert c["xyz"].tolist() == [[7, 3, 3], [7, 7, 7], [8, 3, 3]]
    assert c["label"].tolist() == [0, 1, 0] and c["size"].tolist() == [2, 1] and c["first"].tolist() == [0, 1]
    assert c["box"].tolist() == [[7, 3, 3, 8, 3, 3], [7, 7, 7, 7, 7, 7]]


def test_nothing_wraps_at_the_largest_grid():
    R, y, z = 1 << 21, 5, 9
    vox = [(0, y, z), (R - 1, y, z), (0, y + 1, z), (R - 1, R - 1, R - 1), (R - 2, R - 2, R - 1)]
    for sparse in (True, False):
        f, c = K.components(vox, R, K.FACES, sparse), K.components(vox, R, K.CUBE, sparse)
        assert f["size"].tolist() == [2, 1, 1, 1] and c["size"].tolist() == [2, 1, 2]  # (0, y, z) + (0, y + 1, z); the far corner pair under CUBE only
        assert c["box"][2].tolist() == [R - 2, R - 2, R - 1, R - 1, R - 1, R - 1]


def test_checkerboard():
    for res in (8, 16):
        xyz = checkerboard(res)
        f, c = K.components(xyz, res, K.FACES), K.components(xyz, res, K.CUBE)
        assert len(xyz) == res ** 3 // 2
        assert np.array_equal(f["label"], np.arange(len(xyz))) and (f["size"] == 1).all()
        assert c["size"].tolist() == [len(xyz)] and c["box"].tolist() == [[0, 0, 0] + [res - 1] * 3]


@pytest.mark.parametrize("res,p,element", [(32, 0.1, K.CUBE), (32, 0.3, K.FACES), (8, 0.5, K.FACES), (5, 0.4, K.CUBE)])
def test_against_scipy(res, p, element):
    ndimage = pytest.importorskip("scipy.ndimage")
    g = np.random.default_rng(7).random((res, res, res)) < p
    xyz = np.argwhere(g)
    c = K.components(xyz, res, element)
    raw, n = ndimage.label(g, structure=ndimage.generate_binary_structure(3, 1 if element == K.FACES else 3))
    sx = c["xyz"]
    assert np.array_equal(morton(sx), np.sort(morton(xyz)))
    want = first_appearance(raw[sx[:, 0], sx[:, 1], sx[:, 2]])
    assert len(c["size"]) == n and np.array_equal(c["label"], want)
    assert np.array_equal(c["size"], np.bincount(want)) and c["size"].sum() == len(xyz)
    for k in range(n):
        m = sx[want == k]
        assert c["first"][k] == np.flatnonzero(want == k)[0] and c["box"][k].tolist() == m.min(0).tolist() + m.max(0).tolist()
    if res == 32:  # what tests/test_gpu_components.py asks of these two sets
        sizes, counts = np.unique(c["size"], return_counts=True)
        print("components", n, "largest", c["size"].max(), "tied sizes", (counts > 1).sum())
        assert n >= 500 and c["size"].max() >= 256 and (counts > 1).any()
    s = K.components(xyz, res, element, sparse=True)
    assert all(np.array_equal(c[k], s[k]) for k in c)


def test_selection_rule():
    size = [3, 5, 5, 1, 5, 2]
    assert K.kept_components(size).all()
    assert K.kept_components(size, keep_largest=1).tolist() == [False, True, False, False, False, False]  # the tie goes to the lower label
    assert K.kept_components(size, keep_largest=2).tolist() == [False, True, True, False, False, False]
    assert K.kept_components(size, min_voxels=3).tolist() == [True, True, True, False, True, False]
    assert K.kept_components(size, min_voxels=3, keep_largest=4).tolist() == [True, True, True, False, True, False]
    assert K.kept_components(size, min_voxels=4, keep_largest=4).tolist() == [False, True, True, False, True, False]
    assert not K.kept_components(size, min_voxels=6).any()
    xyz = [(0, 0, 0), (1, 0, 0), (3, 0, 0), (5, 0, 0), (6, 0, 0)]
    at = np.arange(40, dtype=np.uint8).reshape(5, 8)
    kx, ka = K.keep(xyz, at, 8, K.FACES, keep_largest=1)
    assert kx.tolist() == [[0, 0, 0], [1, 0, 0]] and np.array_equal(ka, at[:2])
    assert K.dropped(xyz, 8, K.FACES, min_voxels=2).tolist() == [[3, 0, 0]]
