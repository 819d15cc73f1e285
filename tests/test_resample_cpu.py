"""The numpy model of the affine resampling (tests/resample_expected.py) against itself and against the closed forms, and mvrt_cell_transform_from_world against
the same formula in numpy float64 -- without a GPU.  The dense form evaluates the point rule on every destination cell; the sparse form, which the GPU tests of large
grids are checked against, refines the grid top-down.  They are compared on random transforms of five kinds (rotations, general matrices, 40:1 anisotropic maps,
singular maps, signed permutations) on grids up to 32^3; every named case that is not called empty is asserted non-empty, since two empty lists agree on nothing."""
import numpy as np
import pytest

import massivevoxelraytracing_amd as mv
import resample_expected as E


def random_set(rng, res, fill):
    cells = np.argwhere(rng.random((res, res, res)) < fill)
    if len(cells) == 0:
        cells = np.array([[res // 2] * 3])
    return cells.astype(np.int64), rng.integers(0, 256, size=(len(cells), 8), dtype=np.uint8)


def same(a, b):
    return all(np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype and a[k].shape == b[k].shape for k in ("xyz", "attribs", "source"))


def transforms(rng, rs, rd):
    """(kind, (m, t)) of the five kinds, all mapping the middle of the destination grid near the middle of the source grid"""
    out = []
    for _ in range(3):
        R = E.rotation(rng.normal(size=3), rng.uniform(0, 360))
        out.append(("rotation", E.about_centre(R * (rs / rd), rs, rd, rng.uniform(-1, 1, 3))))
        out.append(("general", E.about_centre(rng.normal(size=(3, 3)) * (rs / rd), rs, rd, rng.uniform(-2, 2, 3))))
        D = np.diag(rng.permutation([4.0, 1.0, 0.1]))  # 40 : 1
        out.append(("anisotropic", E.about_centre(R @ D * (rs / rd), rs, rd)))
        u, v = rng.normal(size=3), rng.normal(size=3)
        out.append(("singular", E.about_centre(np.outer(u, v) * (rs / rd) * 0.5, rs, rd)))  # rank 1
    perms = E.all_signed_permutations(rs)
    if rs == rd:
        out += [("permutation", perms[i][2]) for i in rng.choice(len(perms), 3, replace=False)]
    return out


@pytest.mark.parametrize("rs,rd", [(2, 2), (4, 8), (8, 4), (16, 16), (32, 32), (16, 32), (32, 8)])
def test_sparse_equals_dense_on_random_transforms(rs, rd):
    rng = np.random.default_rng(rs * 100 + rd)
    xyz, at = random_set(rng, rs, 0.2)
    non_empty = 0
    for kind, (m, t) in transforms(rng, rs, rd):
        assert E.transform_ok(m, t)
        d, stats = E.dense(xyz, at, rs, m, t, rd), []
        s = E.sparse(xyz, at, rs, m, t, rd, stats)
        assert same(d, s), kind
        non_empty += len(d["xyz"]) > 0
        if len(d["xyz"]):
            assert np.array_equal(E.point(m, t, d["xyz"]), np.asarray(xyz)[np.argsort(E.morton(xyz))][d["source"]])  # source names the voxel s lands in
            assert (d["attribs"][:, [3, 7]] == 255).all()
    assert non_empty >= 5


def test_identity_and_signed_permutations_are_bijections():
    rng = np.random.default_rng(5)
    for res in (2, 8):
        xyz, at = random_set(rng, res, 0.3)
        order = np.argsort(E.morton(xyz))
        ident = E.dense(xyz, at, res, *E.identity(), res)
        assert len(ident["xyz"]) == len(xyz) > 0 and np.array_equal(ident["xyz"], xyz[order]) and np.array_equal(ident["source"], np.arange(len(xyz)))
        for perm, flips, (m, t) in E.all_signed_permutations(res):
            got = E.dense(xyz, at, res, m, t, res)
            assert same(got, E.sparse(xyz, at, res, m, t, res))
            # closed form: s_i = c_perm[i] or res - 1 - c_perm[i]  <=>  c_perm[i] = s_i or res - 1 - s_i
            c = np.zeros_like(xyz)
            for i in range(3):
                c[:, perm[i]] = res - 1 - xyz[:, i] if flips[i] else xyz[:, i]
            o = np.argsort(E.morton(c))
            assert len(got["xyz"]) == len(xyz) and np.array_equal(got["xyz"], c[o]) and np.array_equal(got["source"], np.argsort(order)[o].astype(np.uint32))


def test_half_and_double_scale_closed_forms():
    rng = np.random.default_rng(6)
    xyz, at = random_set(rng, 8, 0.2)
    order = np.argsort(E.morton(xyz))
    n = len(xyz)
    assert n > 0
    # A = I / 2: s = c >> 1, every voxel becomes a 2x2x2 block
    m, t = E.from_cells(np.eye(3) * 0.5)
    up = E.dense(xyz, at, 8, m, t, 16)
    assert same(up, E.sparse(xyz, at, 8, m, t, 16)) and len(up["xyz"]) == 8 * n
    assert np.array_equal(up["xyz"] >> 1, xyz[order][up["source"]])
    assert np.array_equal(up["source"], np.repeat(np.arange(n, dtype=np.uint32), 8))  # whole blocks, in the order of the voxels
    m4, t4 = E.from_cells(np.eye(3) * 0.25)
    up4 = E.sparse(xyz, at, 8, m4, t4, 32)
    assert len(up4["xyz"]) == 64 * n and np.array_equal(up4["xyz"] >> 2, xyz[order][up4["source"]])
    # A = 2 I: s = 2 c + 1, sub-sampling -- not the count rule of the coarsening
    m, t = E.from_cells(np.eye(3) * 2.0)
    cells = np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), -1).reshape(-1, 3)
    assert np.array_equal(E.point(m, t, cells), 2 * cells + 1)
    full = np.argwhere(np.ones((8, 8, 8), bool))
    down = E.dense(full, np.zeros((512, 8), np.uint8), 8, m, t, 4)
    assert same(down, E.sparse(full, np.zeros((512, 8), np.uint8), 8, m, t, 4)) and len(down["xyz"]) == 64
    odd = xyz[(xyz % 2 == 1).all(1)]
    assert len(E.dense(xyz, at, 8, m, t, 4)["xyz"]) == len(odd)


def test_all_zero_matrix_fills_the_grid_or_leaves_nothing():
    xyz, at = np.array([[3, 5, 7]]), np.full((1, 8), 9, np.uint8)
    zero = np.zeros(9, np.int64)
    hit = E.dense(xyz, at, 16, zero, np.array([3, 5, 7]) * 2 * E.ONE + E.HALF, 16)
    assert len(hit["xyz"]) == 4096 and (hit["source"] == 0).all() and same(hit, E.sparse(xyz, at, 16, zero, np.array([3, 5, 7]) * 2 * E.ONE + E.HALF, 16))
    miss = E.sparse(xyz, at, 16, zero, np.array([3, 5, 6]) * 2 * E.ONE, 16)
    assert len(miss["xyz"]) == 0 and same(miss, E.dense(xyz, at, 16, zero, np.array([3, 5, 6]) * 2 * E.ONE, 16))
    outside = E.sparse(xyz, at, 16, E.identity()[0], np.full(3, 64 * 2 * E.ONE), 16)
    assert len(outside["xyz"]) == 0


def test_floor_is_towards_minus_infinity():
    m = np.zeros(9, np.int64)
    for p, want in ((-1, -1), (-(1 << 25), -1), (-(1 << 25) - 1, -2), (0, 0), ((1 << 25) - 1, 0), (1 << 25, 1)):
        assert E.point(m, np.array([p, 0, 0]), [[0, 0, 0]])[0, 0] == want


# ---- mvrt_cell_transform_from_world ---------------------------------------------------------------------------------------------------------------------------
def world_of(W, w):
    return np.concatenate([np.asarray(W, np.float64).reshape(3, 3), np.asarray(w, np.float64).reshape(3, 1)], 1)


def test_from_world_is_exact_where_everything_is_representable():
    ident = mv.cell_transform_from_world(world_of(np.eye(3), [0, 0, 0]), [0, 0, 0], 0.25, [0, 0, 0], 0.25)
    assert ident.structBytes == 104 and ident.reserved == 0
    m, t = ident.arrays()
    assert np.array_equal(m, E.identity()[0]) and not t.any()
    for perm, flips, _ in E.all_signed_permutations(8):
        W = np.zeros((3, 3))
        for i in range(3):
            W[i, perm[i]] = -1.0 if flips[i] else 1.0
        for sd, dd, w, sl, dl in ((0.5, 0.5, [0, 0, 0], [0, 0, 0], [0, 0, 0]), (0.25, 2.0, [3, -8, 16], [1, 2, -4], [-2, 0.5, 8]), (4.0, 0.125, [0, 64, -1], [0.25, 0, 0], [0, 0, 3])):
            got = mv.cell_transform_from_world(world_of(W, w), sl, sd, dl, dd).arrays()
            fm, ft = E.from_world(world_of(W, w), sl, sd, dl, dd)
            assert (fm == np.rint(fm)).all() and (ft == np.rint(ft)).all()  # the case is exact
            assert np.array_equal(got[0], fm.astype(np.int64)) and np.array_equal(got[1], ft.astype(np.int64))
    # a mirror about the grid centre through world space is the signed permutation of the model: W = -I about the centre of an 8^3 grid of dps 1 at the origin
    got = mv.cell_transform_from_world(world_of(-np.eye(3), [8, 8, 8]), [0, 0, 0], 1.0, [0, 0, 0], 1.0).arrays()
    want = E.signed_permutation((0, 1, 2), (1, 1, 1), 8)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # power-of-two scales: a set twice as large in world space on the same lattice is A = I / 2
    got = mv.cell_transform_from_world(world_of(2 * np.eye(3), [0, 0, 0]), [0, 0, 0], 0.5, [0, 0, 0], 0.5).arrays()
    assert np.array_equal(got[0], E.from_cells(np.eye(3) * 0.5)[0]) and not got[1].any()


def test_from_world_is_within_one_unit_otherwise():
    rng = np.random.default_rng(9)
    for _ in range(200):
        W = E.rotation(rng.normal(size=3), rng.uniform(0, 360)) * rng.uniform(0.2, 5.0) if rng.random() < 0.5 else rng.normal(size=(3, 3))
        w, sl, dl = rng.uniform(-3, 3, 3), rng.uniform(-3, 3, 3).astype(np.float32), rng.uniform(-3, 3, 3).astype(np.float32)
        sd, dd = np.float32(rng.uniform(0.01, 0.1)), np.float32(rng.uniform(0.01, 0.1))
        fm, ft = E.from_world(world_of(W, w), sl, sd, dl, dd)
        if np.abs(fm).max() > 2.0 ** 30 or np.abs(ft).max() > 2.0 ** 52:
            continue
        m, t = mv.cell_transform_from_world(world_of(W, w), sl, sd, dl, dd).arrays()
        # the double computation carries a relative error near 1e-15 on magnitudes below 2^30 (m) -- far below one unit -- so the two roundings can differ only by
        # landing on opposite sides of a tie; t reaches 2^52 in range, here it stays below 2^40, where 1e-15 relative is still far below one unit
        assert np.abs(m - np.rint(fm)).max() <= 1 and np.abs(ft).max() < 2.0 ** 40 and np.abs(t - np.rint(ft)).max() <= 1


def test_from_world_refusals():
    ok = dict(world=world_of(np.eye(3), [0, 0, 0]), src_lower=[0, 0, 0], src_dps=1.0, dst_lower=[0, 0, 0], dst_dps=1.0)
    mv.cell_transform_from_world(**ok)
    singular = world_of([[1, 2, 3], [2, 4, 6], [0, 0, 1]], [0, 0, 0])
    with pytest.raises(mv.MvrtError, match="singular"):
        mv.cell_transform_from_world(**dict(ok, world=singular))
    with pytest.raises(mv.MvrtError, match="singular"):
        mv.cell_transform_from_world(**dict(ok, world=world_of(np.zeros((3, 3)), [0, 0, 0])))
    for bad in (np.nan, np.inf):
        with pytest.raises(mv.MvrtError, match="not finite"):
            mv.cell_transform_from_world(**dict(ok, world=world_of(np.eye(3), [0, bad, 0])))
        with pytest.raises(mv.MvrtError, match="not finite"):
            mv.cell_transform_from_world(**dict(ok, src_lower=[bad, 0, 0]))
        with pytest.raises(mv.MvrtError, match="dps"):
            mv.cell_transform_from_world(**dict(ok, dst_dps=bad))
    for bad in (0.0, -1.0):
        with pytest.raises(mv.MvrtError, match="dps"):
            mv.cell_transform_from_world(**dict(ok, src_dps=bad))
    with pytest.raises(mv.MvrtError, match="out of range"):
        mv.cell_transform_from_world(**dict(ok, world=world_of(np.eye(3) / 65.0, [0, 0, 0])))  # an entry of 65 > 64
    mv.cell_transform_from_world(**dict(ok, world=world_of(np.eye(3) / 64.0, [0, 0, 0])))  # 64 is the limit itself
    with pytest.raises(mv.MvrtError, match="out of range"):
        mv.cell_transform_from_world(**dict(ok, dst_lower=[2.0 ** 28, 0, 0]))  # t = 2^28 * 2^25 > 2^52
    with pytest.raises(mv.MvrtError, match="singular"):
        mv.cell_transform_from_world(**dict(ok, world=world_of(np.eye(3) * 1e-200, [0, 0, 0])))  # det underflows to 0
