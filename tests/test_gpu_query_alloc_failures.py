"""Every device allocation of mvrt_svo_nearest_voxels, mvrt_svo_nearest_between and mvrt_svo_transfer_attributes is made to fail in turn
(mvrt_test_fail_allocation), as tests/test_gpu_enclosed_nearest_alloc_failures.py does for the enclosed cells.  The listings only read their handles: each
failure names the hook, leaves the octrees bit-identical and the caller's arrays untouched, and mvrt_test_allocation_state returns to where it was.  The
transfer is the attribute-only edit: it writes in place behind its last allocation, so every failure leaves dst as it was."""
import numpy as np
import pytest

import query_expected as Q
from alloc_sweep import filled, mv, same, sweep_reader  # noqa: F401 (mv: the fixture)
from voxel_sets import DPS, LOWER

pytestmark = pytest.mark.gpu

RES = 32


@pytest.fixture(scope="module")
def sets():
    rng = np.random.default_rng(31)
    a = np.argwhere(rng.random((RES, RES, RES)) < 0.03).astype(np.uint32)
    b = np.argwhere(rng.random((RES, RES, RES)) < 0.02).astype(np.uint32)
    return a, rng.integers(0, 256, (len(a), 8), dtype=np.uint8), b, rng.integers(0, 256, (len(b), 8), dtype=np.uint8)


def build(mv, xyz, at, svo=None):
    svo = mv.IntersectorOctreeGPU() if svo is None else svo
    svo.build_voxels(xyz, at, origin=LOWER, dps=DPS, gridRes=RES)
    return svo


def test_each_allocation_of_the_queries_fails_in_turn(mv, sets):
    xa, aa, xb, ab = sets
    svo = build(mv, xa, aa)
    q = np.random.default_rng(2).integers(-5, RES + 5, (1000, 3)).astype(np.int32)
    qd = mv.DeviceArray.from_host(q)
    d2, near, at = filled(mv, len(q), np.uint64), filled(mv, len(q), np.uint32), filled(mv, (len(q), 8), np.uint8)
    total, _ = sweep_reader(mv, lambda: svo.nearest_voxels_device(len(q), qd, dist2=d2[0], nearest=near[0], attribs=at[0]), [svo], [d2, near, at], 1)
    print("nearest_voxels: allocations failed in turn:", total)
    want = Q.nearest_voxels(xa, aa, q)
    assert np.array_equal(d2[0].to_host(), want["dist2"]) and np.array_equal(near[0].to_host(), want["nearest"]) and np.array_equal(at[0].to_host(), want["attribs"])


def test_each_allocation_of_the_two_set_call_fails_in_turn(mv, sets):
    xa, aa, xb, ab = sets
    a, b = build(mv, xa, aa), build(mv, xb, ab)
    n = a.info().numberOfVoxels
    d2, near = filled(mv, n, np.uint64), filled(mv, n, np.uint32)
    total, _ = sweep_reader(mv, lambda: a.nearest_between_device(b, (1, 2, -1), capacity=n, dist2=d2[0], nearest=near[0]), [a, b], [d2, near], 1)
    summary, _ = sweep_reader(mv, lambda: a.nearest_between_device(b, (1, 2, -1)), [a, b], [d2, near], 2)  # the summary call keeps the distances in scratch
    print("nearest_between: allocations failed in turn:", total, "summary call:", summary)
    got = a.nearest_between_device(b, (1, 2, -1), capacity=n, dist2=d2[0], nearest=near[0])
    want = Q.nearest_between(xa, xb, (1, 2, -1))
    assert got == {k: want[k] for k in ("n", "maxDist2", "farthest", "zero", "beyond")}
    assert np.array_equal(d2[0].to_host(), want["dist2"]) and np.array_equal(near[0].to_host(), want["nearest"])


def test_each_allocation_of_the_transfer_fails_in_turn(mv, sets):
    xa, aa, xb, ab = sets
    src = build(mv, xb, ab)
    x, new, taken, changed = Q.transferred(xa, Q.alpha255(aa), xb, ab, (0, 1, 0), 3, 3)  # (build_voxels stores the alpha bytes as 255)
    assert 0 < taken.sum() < len(taken)
    twin = build(mv, xa, aa)
    twin.edit_voxels(x[taken].astype(np.uint32), new[taken])
    expected = twin.download(want_morton=True)
    dst = build(mv, xa, aa)
    # the walk's 5, the list's 4, the edit's own
    total, result = sweep_reader(mv, lambda: dst.transfer_attributes(src, (0, 1, 0), 3), [dst, src], [], 15, reset=lambda: build(mv, xa, aa, dst))
    print("transfer_attributes: allocations failed in turn:", total)
    assert result == (changed, int((~taken).sum())) and same(dst.download(want_morton=True), expected)
