"""The numpy model of the two-set operations (tests/combine_expected.py) against dense boolean grids, without a GPU: the GPU tests compare bit for bit with the
model, so the model itself is held to a second, independent formulation here -- occupancy and attribute grids indexed [x, y, z], the shift done by slicing (no
roll, nothing wraps), the operators as numpy's boolean operators -- at gridRes 2, 4 and 16, for all four ops and offsets that clip nothing, something and
everything; and to the identities of the set algebra."""
import itertools

import numpy as np
import pytest

import combine_expected as E
from surface_expected import morton


def random_set(res, density, seed):
    rng = np.random.default_rng(seed)
    occ = rng.random((res, res, res)) < density
    if not occ.any():
        occ[rng.integers(res), rng.integers(res), rng.integers(res)] = True
    xyz = np.argwhere(occ)
    rng.shuffle(xyz)  # (the model may not depend on the order of its input)
    return xyz, rng.integers(0, 256, size=(len(xyz), 8), dtype=np.uint8)


def dense(xyz, attribs, res):
    occ, at = np.zeros((res,) * 3, bool), np.zeros((res,) * 3 + (8,), np.uint8)
    occ[tuple(np.asarray(xyz).T)] = True
    at[tuple(np.asarray(xyz).T)] = attribs
    return occ, at


def shifted(occ, at, res_a, offset):
    """the grids of b moved by offset into a grid of res_a cells per axis, by slicing; returns (occupancy, attributes, clipped)"""
    out, out_at = np.zeros((res_a,) * 3, bool), np.zeros((res_a,) * 3 + (8,), np.uint8)
    src, dst = [], []
    for k in range(3):
        lo, hi = max(0, -offset[k]), min(occ.shape[k], res_a - offset[k])  # the cells of b that stay inside
        if lo >= hi:
            return out, out_at, int(occ.sum())
        src.append(slice(lo, hi))
        dst.append(slice(lo + offset[k], hi + offset[k]))
    out[tuple(dst)] = occ[tuple(src)]
    out_at[tuple(dst)] = at[tuple(src)]
    return out, out_at, int(occ.sum() - out.sum())


def dense_combine(a, b, res_a, res_b, op, offset, flags):
    oa, ata = dense(a[0], a[1], res_a)
    ob, atb, clipped = shifted(*dense(b[0], b[1], res_b), res_a, offset)
    atb[..., 3] = 255
    atb[..., 7] = 255
    occ = {E.UNION: oa | ob, E.INTERSECTION: oa & ob, E.DIFFERENCE: oa & ~ob, E.XOR: oa ^ ob}[op]
    at = np.where(oa[..., None], ata, atb)
    if flags & E.ATTRIB_B:
        at = np.where(ob[..., None], atb, ata)
    xyz = np.argwhere(occ)
    xyz = xyz[np.argsort(morton(xyz), kind="stable")]
    idx = tuple(xyz.T)
    source = oa[idx].astype(np.uint8) | (ob[idx].astype(np.uint8) << 1)
    return {"xyz": xyz.astype(np.uint32), "attribs": at[idx].reshape(-1, 8), "source": source.astype(np.uint8), "overlap": int((oa & ob).sum()), "clipped": clipped}


def assert_equal(got, want):
    assert got["xyz"].dtype == np.uint32 and got["attribs"].dtype == np.uint8 and got["source"].dtype == np.uint8
    for k in ("xyz", "attribs", "source"):
        assert np.array_equal(got[k], want[k]), k
    assert (got["overlap"], got["clipped"]) == (want["overlap"], want["clipped"])


def offsets_of(res):
    """nothing clipped, one layer, half the grid, everything -- in both directions and on mixed axes"""
    return [(0, 0, 0), (1, 0, 0), (0, -1, 0), (0, 0, res // 2), (-1, 1, -1), (res - 1, 0, 0), (res, 0, 0), (0, -res, 0), (res + 3, -res, 1)]


@pytest.mark.parametrize("res", [2, 4, 16])
def test_model_against_dense_grids(res):
    a, b = random_set(res, 0.4, res), random_set(res, 0.4, res + 100)
    seen = set()
    for op, off, flags in itertools.product(E.OPS, offsets_of(res), (0, E.ATTRIB_B)):
        got = E.combine(a[0], a[1], b[0], b[1], res, op, off, flags)
        assert_equal(got, dense_combine(a, b, res, res, op, off, flags))
        seen.add("all" if got["clipped"] == len(b[0]) else "some" if got["clipped"] else "none")
        assert len(got["xyz"]) == {E.UNION: len(a[0]) + len(b[0]) - got["clipped"] - got["overlap"], E.INTERSECTION: got["overlap"], E.DIFFERENCE: len(a[0]) - got["overlap"],
                                   E.XOR: len(a[0]) + len(b[0]) - got["clipped"] - 2 * got["overlap"]}[op]
    assert seen == {"all", "some", "none"}
    assert_equal(E.combine(a[0], a[1], b[0], b[1], res, E.UNION, None), E.combine(a[0], a[1], b[0], b[1], res, E.UNION, (0, 0, 0)))  # None = zero


@pytest.mark.parametrize("res_a,res_b", [(16, 4), (4, 16), (2, 16)])
def test_grids_of_different_size(res_a, res_b):
    a, b = random_set(res_a, 0.3, 5), random_set(res_b, 0.3, 6)
    for op, off in itertools.product(E.OPS, [(0, 0, 0), (3, 1, 2), (-2, 0, -1), (res_a - 1, res_a - 1, res_a - 1), (-res_b, 0, 0)]):
        assert_equal(E.combine(a[0], a[1], b[0], b[1], res_a, op, off, E.ATTRIB_B), dense_combine(a, b, res_a, res_b, op, off, E.ATTRIB_B))


def codes_of(r):
    return morton(r["xyz"])


@pytest.mark.parametrize("res", [2, 4, 16])
def test_identities(res):
    a, b = random_set(res, 0.5, 11), random_set(res, 0.5, 12)
    for off in offsets_of(res):
        r = {op: E.combine(a[0], a[1], b[0], b[1], res, op, off) for op in E.OPS}
        # XOR = UNION \ INTERSECTION, with the attributes the union gives those voxels
        keep = ~np.isin(codes_of(r[E.UNION]), codes_of(r[E.INTERSECTION]))
        assert np.array_equal(r[E.XOR]["xyz"], r[E.UNION]["xyz"][keep]) and np.array_equal(r[E.XOR]["attribs"], r[E.UNION]["attribs"][keep])
        assert np.array_equal(r[E.XOR]["source"], r[E.UNION]["source"][keep]) and not (r[E.XOR]["source"] == 3).any()
        # A \ B' = A n ( grid \ B' )
        cb, _, _ = E.translate(b[0], b[1], res, off)
        every = np.argwhere(np.ones((res,) * 3, bool))
        rest = every[~np.isin(morton(every), cb)]
        if len(rest):
            inter = E.combine(a[0], a[1], rest, np.zeros((len(rest), 8), np.uint8), res, E.INTERSECTION)
            assert np.array_equal(inter["xyz"], r[E.DIFFERENCE]["xyz"]) and np.array_equal(inter["attribs"], r[E.DIFFERENCE]["attribs"])
        else:
            assert len(r[E.DIFFERENCE]["xyz"]) == 0
        assert (r[E.DIFFERENCE]["source"] == 1).all() and (r[E.INTERSECTION]["source"] == 3).all()
        # ATTRIB_B has no effect on difference and xor
        for op in (E.DIFFERENCE, E.XOR):
            assert_equal(E.combine(a[0], a[1], b[0], b[1], res, op, off, E.ATTRIB_B), r[op])


def test_union_commutes_as_a_set_but_not_in_its_attributes():
    res = 16
    a, b = random_set(res, 0.5, 21), random_set(res, 0.5, 22)
    ab = E.combine(a[0], a[1], b[0], b[1], res, E.UNION)
    ba = E.combine(b[0], b[1], a[0], a[1], res, E.UNION)
    assert np.array_equal(ab["xyz"], ba["xyz"]) and ab["overlap"] == ba["overlap"] > 0
    both = ab["source"] == 3
    assert np.array_equal(both, ba["source"] == 3) and np.array_equal(ab["source"][~both], 3 - ba["source"][~both])
    assert not np.array_equal(ab["attribs"][both], ba["attribs"][both])  # each keeps its own first operand's bytes
    # ... and ATTRIB_B on one side gives the colour and emission of the other side's plain union, with alpha 255
    abf = E.combine(a[0], a[1], b[0], b[1], res, E.UNION, None, E.ATTRIB_B)
    assert np.array_equal(abf["attribs"][both][:, [0, 1, 2, 4, 5, 6]], ba["attribs"][both][:, [0, 1, 2, 4, 5, 6]]) and (abf["attribs"][both][:, [3, 7]] == 255).all()


@pytest.mark.parametrize("op", E.OPS)
@pytest.mark.parametrize("flags", [0, E.ATTRIB_B])
def test_edit_lists_reproduce_the_result(op, flags):
    """the SET / REMOVE batch, applied to A as a plain dictionary edit, gives the model's result: what the GPU test asks of mvrt_svo_edit_voxels on a twin handle"""
    res = 16
    a, b = random_set(res, 0.4, 31), random_set(res, 0.4, 32)
    for off in [(0, 0, 0), (2, -1, 0), (res - 1, 0, 0), (res, 0, 0)]:
        want = E.combine(a[0], a[1], b[0], b[1], res, op, off, flags)
        xyz, at, ops, (added, removed) = E.edit_lists(a[0], a[1], b[0], b[1], res, op, off, flags)
        cells = {tuple(int(c) for c in v): bytes(t) for v, t in zip(a[0], a[1])}
        for v, t, o in zip(xyz, at, ops):
            if o == E.SET:
                cells[tuple(int(c) for c in v)] = bytes(t)
            else:
                del cells[tuple(int(c) for c in v)]
        assert len(cells) == len(want["xyz"]) == len(a[0]) + added - removed
        assert all(cells[tuple(int(c) for c in v)] == bytes(t) for v, t in zip(want["xyz"], want["attribs"]))
