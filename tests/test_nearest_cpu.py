"""The model of the nearest voxel of the enclosed cells (tests/nearest_expected.py) without a GPU: against the model of the distance band
(ball_expected.distance_cells with the largest radius) on the enclosed cells both list, d2 = 1 exactly for the cells with a voxel face neighbour, the bound
d2 < 2^20 on the sets used, the tie rule on shapes whose answer is known by hand, and the bunny at 64^3 with the oracle's voxelizer."""
import numpy as np

import ball_expected as B
import fill_expected as F
import nearest_expected as N
import surface_expected as S
from common import bunny_tris
from voxel_sets import cavities, colours, shell


def assert_face_neighbours_are_at_distance_one(xyz, want, res):
    occupied = set(map(tuple, np.asarray(xyz).tolist()))
    steps = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    touching = np.array([any((c[0] + d[0], c[1] + d[1], c[2] + d[2]) in occupied for d in steps) for c in want["xyz"].tolist()], bool)
    assert touching.any() and np.array_equal(want["dist2"] == 1, touching) and want["dist2"].min() >= 1


def test_model_against_the_band_model_and_distance_one():
    for xyz, res in cavities():
        at = colours(len(xyz))
        want = N.enclosed_nearest(xyz, at, res)
        band = B.distance_cells(xyz, at, res, 1024)
        index = {int(c): i for i, c in enumerate(S.morton(band["xyz"]))}
        codes = S.morton(want["xyz"])
        assert len(want["xyz"]) > 100 and want["dist2"].max() < 1024 < 1 << 20 and all(int(c) in index for c in codes)
        rows = np.array([index[int(c)] for c in codes], np.int64)
        for k in ("dist2", "nearest", "attribs"):
            assert np.array_equal(band[k][rows], want[k]), k
        assert (want["attribs"][:, 3] == 255).all() and (want["attribs"][:, 7] == 255).all()
        assert_face_neighbours_are_at_distance_one(xyz, want, res)
        e = F.enclosed(xyz, res)
        assert np.array_equal(e["xyz"], want["xyz"]) and np.array_equal(e["region"], want["region"]) and e["nRegions"] == want["nRegions"]


def test_ties_go_to_the_lowest_vindex():
    want = N.enclosed_nearest(shell(0, 3), None, 4)  # one cell, six voxels at distance 1: (1, 1, 0) has the lowest code, behind the codes 0, 1, 2
    assert want["xyz"].tolist() == [[1, 1, 1]] and want["dist2"].tolist() == [1] and want["nearest"].tolist() == [3]
    cage = shell(1, 6)
    want = N.enclosed_nearest(cage, None, 8)
    order = cage[np.argsort(S.morton(cage), kind="stable")]
    centre = want["xyz"].tolist().index([3, 3, 3])
    assert want["dist2"][centre] == 4 and order[want["nearest"][centre]].tolist() == [3, 3, 1]  # of the six at distance 2 the one below: z is the highest bit
    corner = want["xyz"].tolist().index([2, 2, 2])
    assert want["dist2"][corner] == 1 and order[want["nearest"][corner]].tolist() == [2, 2, 1]


def test_the_fill_keeps_the_voxels_and_adds_the_cells_with_their_attributes():
    xyz, res = next(cavities())
    at = colours(len(xyz), 3)
    want = N.enclosed_nearest(xyz, at, res)
    fx, fa = N.filled(xyz, at, res)
    assert len(fx) == len(xyz) + len(want["xyz"]) and np.array_equal(S.morton(fx), np.sort(S.morton(fx)))
    added = np.isin(S.morton(fx), S.morton(want["xyz"]))
    assert np.array_equal(fx[added], want["xyz"]) and np.array_equal(fa[added], want["attribs"])
    assert np.array_equal(fa[~added], at[np.argsort(S.morton(xyz), kind="stable")])  # verbatim


def test_bunny_at_64_with_the_oracles_voxelizer():
    from oracle import oracle as O
    O.build()
    tris = bunny_tris()
    v = tris.reshape(-1, 3)
    lo = v.min(0)
    dps = np.float32((v.max(0) - lo).max() / np.float32(64))
    xyz = S.decode(np.unique(O.voxelize(tris, lo, dps, 64, six_separating=True)[0]))
    want = N.enclosed_nearest(xyz, colours(len(xyz), 12), 64)
    assert (len(xyz), len(want["xyz"]), want["nRegions"]) == (8516, 48162, 3)
    print("deepest d2", want["dist2"].max())
    assert 1 <= want["dist2"].min() and want["dist2"].max() < 32 * 32 * 3  # inside a 64^3 grid
    assert_face_neighbours_are_at_distance_one(xyz, want, 64)
    # the one-cell and two-cell regions lie against the shell
    sizes = np.bincount(want["region"])
    assert (want["dist2"][np.isin(want["region"], np.flatnonzero(sizes <= 2))] == 1).all()
