"""What tests/test_gpu_*_alloc_failures.py share: the two contracts of include/mvrt.h, "What a failed call leaves behind", each stated once.  A sweep runs the call
once for the number of its allocations, then with each of them failing in turn (mvrt_test_fail_allocation).  After every failure the error names the hook, the
hook has disarmed itself, mvrt_test_allocation_state is where it was and every handle that is only read is bit-identical.  sweep_reader is for the calls that
only read their handles (listings, queries, surface calls): the caller's arrays keep their canary too.  sweep_edit is for the calls that replace an octree: the
destination is the old octree, whole, up to the adoption of the new arrays and an empty handle from there on.  tests/test_alloc_sweep_cpu.py runs both against a
fake library and sees each of their assertions fire."""
import numpy as np
import pytest

from fixtures import mv  # noqa: F401 (the fixture, for the sweep files)
from voxel_sets import filled, same  # noqa: F401 (filled: for the sweep files)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def with_morton(handle):
    return handle.download(want_morton=True)


def snapshot(handle, download=with_morton):
    return download(handle), bytes(handle.info())


def unchanged(handle, snap, download=with_morton):
    return bytes(handle.info()) == snap[1] and same(download(handle), snap[0])


def fail_kth(mv, k, call):
    mv.set_test_fail_allocation(k)
    with pytest.raises(mv.MvrtError, match="mvrt_test_fail_allocation"):
        call()
    assert mv.lib().mvrt_test_fail_allocation(0) == 0, k  # the hook has disarmed itself


def sweep_reader(mv, call, handles, arrays, least, reset=None, download=with_morton):
    """handles: what the call reads; arrays: the [(device, canary)] it writes, behind its last allocation; reset(): for a call that writes into a handle in place,
    behind its last allocation, puts the bytes from before the call back.  Returns (allocations, the call's result)."""
    whole, state = [snapshot(h, download) for h in handles], mv.allocation_state()
    result = call()
    total = mv.allocation_state()[2] - state[2]
    assert total >= least and mv.allocation_state()[:2] == state[:2]
    for d, h in arrays:  # back to the canary for the sweep
        mv.lib().mvrt_memcpy_h2d(d.ptr, h.ctypes.data, d.nbytes, None)
    for k in range(1, total + 1):
        if reset:
            reset()
        fail_kth(mv, k, call)
        assert mv.allocation_state()[:2] == state[:2], k  # nothing leaked
        for i, (h, snap) in enumerate(zip(handles, whole)):
            assert unchanged(h, snap, download), (k, i)
        for i, (d, h) in enumerate(arrays):
            assert np.array_equal(bits(d.to_host()), bits(h)), (k, i)
    if reset:
        reset()
    assert call() == result
    return total, result


def sweep_edit(mv, call, dst, reset, base, refused, least, bystanders=(), live_when_empty=(0, 0)):
    """call() replaces the octree of dst; reset() puts back what it held, as on entry; base: mvrt_test_allocation_state()[:2] from before any handle of the test;
    refused(): a reader of dst; bystanders: handles the call only reads; live_when_empty: (buffers, bytes) over base that the other handles hold alone.
    Returns (allocations, how many of them, the first ones, kept the old octree)."""
    def live():
        return tuple(a - b for a, b in zip(mv.allocation_state()[:2], base))

    held, old, whole = live(), snapshot(dst), [snapshot(h) for h in bystanders]
    before = mv.allocation_state()[2]
    call()
    total = mv.allocation_state()[2] - before
    expected = snapshot(dst)
    assert total >= least
    ends = []
    for k in range(1, total + 1):
        reset()
        assert bytes(dst.info()) == old[1] and live() == held, k
        fail_kth(mv, k, call)
        now = live()
        for i, (h, snap) in enumerate(zip(bystanders, whole)):
            assert unchanged(h, snap), (k, i)
        if dst.info().numberOfNodes == 0:  # behind the adoption: an empty handle that every reader refuses
            ends.append("empty")
            assert now == live_when_empty, k
            with pytest.raises(mv.MvrtError, match="no octree"):
                refused()
        else:
            ends.append("old")
            assert now == held, k
            assert unchanged(dst, old), k
    assert ends == sorted(ends, reverse=True) and ends[0] == "old" and ends[-1] == "empty", ends  # the old octree up to one point of the call, none from there on
    reset()
    call()
    assert unchanged(dst, expected)
    return total, ends.count("old")
