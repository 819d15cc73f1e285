"""tests/alloc_sweep.py against a library made of Python: a call of N allocations through the bookkeeping of csrc/devbuf.h, with the adoption before allocation
ADOPT where it edits.  The well-behaved library passes both sweeps; each FAULT below, alone, is one way a call can break "What a failed call leaves behind"
(include/mvrt.h) or a test can hold the sweep wrongly, and makes the sweep fail.  mvrt_test_fail_allocation returns a status, not what was armed, so a hook
left armed shows as it would on the GPU: the call returns where it should have raised."""
import ctypes

import numpy as np
import pytest

from alloc_sweep import filled, sweep_edit, sweep_reader

N, ADOPT = 7, 4
FAULTS = {"a buffer leaks", "bytes leak", "the octree changes", "the info changes", "a caller array is written early", "the error lacks the hook's name",
          "the hook is left armed", "a bystander changes", "fewer allocations than least", "the unhooked call returns something else",
          "old follows empty", "never empty", "never old", "the empty handle holds buffers", "the empty handle is read", "the final octree differs"}


class FakeError(RuntimeError):
    pass


class Info(ctypes.Structure):
    _fields_ = [("numberOfNodes", ctypes.c_uint32), ("numberOfVoxels", ctypes.c_uint32)]


class Library:
    """the package and its C library in one: the names tests/alloc_sweep.py uses"""
    MvrtError = FakeError

    def __init__(self, fault=None):
        assert fault is None or fault in FAULTS
        self.fault, self.buffers, self.bytes, self.attempts, self.armed, self.calls, self.arrays = fault, 0, 0, 0, 0, 0, {}
        self.DeviceArray = type("DeviceArray", (Array,), {"library": self})

    def lib(self):
        return self

    def allocation_state(self):
        return self.buffers, self.bytes, self.attempts

    def set_test_fail_allocation(self, nth):
        assert self.mvrt_test_fail_allocation(nth) == 0

    def mvrt_test_fail_allocation(self, nth):
        self.armed = max(nth, 0)
        return 0

    def mvrt_memcpy_h2d(self, ptr, src, nbytes, stream):
        self.arrays[ptr].bytes[:] = np.frombuffer(ctypes.string_at(src, nbytes), np.uint8)

    def alloc(self, nbytes):  # DevBuf::alloc
        self.attempts += 1
        if self.armed > 0:
            self.armed -= 1
            if self.armed == 0:
                raise FakeError("out of memory" if self.fault == "the error lacks the hook's name" else "allocation of %d bytes refused by mvrt_test_fail_allocation" % nbytes)
        self.buffers += 1
        self.bytes += nbytes

    def free(self, sizes):
        self.buffers -= len(sizes)
        self.bytes -= sum(sizes)

    def scratch(self, n, before=lambda i: None):
        """n allocations, freed again where one of them fails; returns their sizes"""
        if self.fault == "the hook is left armed" and self.armed == n:
            n -= 1  # (a hooked call that skips its last allocation)
        if self.fault == "fewer allocations than least":
            n -= 1
        held = []
        try:
            for i in range(n):
                before(i)
                self.alloc(64 + i)
                held.append(64 + i)
        except FakeError:
            self.failed = len(held)  # (the index of the allocation that failed)
            self.free(held[1:] if self.fault == "a buffer leaks" else held)
            self.bytes += 8 if self.fault == "bytes leak" else 0
            raise
        return held


class Array:
    def __init__(self, host):
        self.bytes, self.dtype, self.shape = np.ascontiguousarray(host).view(np.uint8).reshape(-1).copy(), host.dtype, host.shape
        self.ptr, self.nbytes = 0x1000 + len(self.library.arrays), host.nbytes
        self.library.arrays[self.ptr] = self

    @classmethod
    def from_host(cls, host):
        return cls(host)

    def to_host(self):
        return self.bytes.view(self.dtype).reshape(self.shape).copy()


class Octree:
    """a handle: two buffers while it holds an octree, none while it is empty"""

    def __init__(self, library, seed=None):
        self.library, self.held, self.nodes, self.voxels = library, [], np.zeros(0, np.uint32), 0
        if seed is not None:
            self.build(seed)

    def build(self, seed):
        self.library.alloc(160)
        self.library.alloc(160)
        self.adopt(np.arange(seed, seed + 40, dtype=np.uint32), [160, 160])

    def adopt(self, nodes, held):
        self.release()
        self.nodes, self.voxels, self.held = nodes, len(nodes) // 2, held

    def release(self):
        self.library.free(self.held)
        self.nodes, self.voxels, self.held = np.zeros(0, np.uint32), 0, []

    def info(self):
        return Info(len(self.nodes), self.voxels)

    def download(self, want_morton=False):
        return (self.nodes.copy(), self.nodes[::2].copy()) + ((self.nodes[1::2].copy(),) if want_morton else ())

    def disturb(self, fault):
        if fault == "the octree changes":
            self.nodes[3] ^= 1
        if fault == "the info changes":
            self.voxels += 1

    def listing(self, other, out):
        """reads both handles; writes the caller's array behind the last of its N allocations"""
        lib = self.library
        if not len(self.nodes) and lib.fault != "the empty handle is read":
            raise FakeError("this handle holds no octree")
        lib.calls += 1

        def early(i):
            if i == N - 1 and lib.fault == "a caller array is written early":
                out.bytes[:] = 1
        try:
            lib.free(lib.scratch(N, early))
        except FakeError:
            self.disturb(lib.fault)
            if lib.fault == "a bystander changes":
                other.nodes[5] += 1
            raise
        out.bytes[:] = 2
        return int(self.nodes.sum()) + (lib.calls if lib.fault == "the unhooked call returns something else" else 0)

    def recolour(self, other):
        """the attribute-only edit: writes in place, behind the last of its N allocations"""
        try:
            self.library.free(self.library.scratch(N))
        except FakeError:
            self.disturb(self.library.fault)
            raise
        self.nodes[1::2] = other.nodes[1::2]

    def edit(self, other):
        """replaces its octree by one made of other's; releases the old one before allocation ADOPT"""
        lib = self.library
        lib.calls += 1
        adopt = {"never empty": N, "never old": 0}.get(lib.fault, ADOPT)
        old = self.nodes.copy()

        def before(i):
            if i == adopt:
                self.release()
        try:
            held = lib.scratch(N, before)
        except FakeError:
            if len(self.nodes):
                self.disturb(lib.fault)
            elif lib.fault == "the empty handle holds buffers" or lib.fault == "old follows empty" and lib.failed == N - 1:
                lib.buffers, lib.bytes = lib.buffers + 2, lib.bytes + 320
                if lib.fault == "old follows empty":
                    self.adopt(old, [160, 160])
            if lib.fault == "a bystander changes":
                other.nodes[5] += 1
            raise
        lib.free(held[:-2])
        self.adopt(other.nodes + (lib.calls if lib.fault == "the final octree differs" else 1), held[-2:])


@pytest.mark.parametrize("fault", [None, "in place"] + sorted(FAULTS - {"old follows empty", "never empty", "never old", "the empty handle holds buffers",
                                                                         "the empty handle is read", "the final octree differs"}))
def test_reader_contract(fault):
    in_place = fault == "in place"
    lib = Library(None if in_place else fault)
    a, b = Octree(lib, 100), Octree(lib, 200)
    out = filled(lib, (5, 3), np.uint32)

    def sweep():
        if in_place:
            return sweep_reader(lib, lambda: a.recolour(b), [a, b], [], N, reset=lambda: a.build(100))
        return sweep_reader(lib, lambda: a.listing(b, out[0]), [a, b], [out], N)

    if fault in FAULTS:
        with pytest.raises((AssertionError, pytest.fail.Exception)):
            sweep()
        return
    assert sweep() == (N, None if in_place else int(a.nodes.sum()))
    assert np.array_equal(a.nodes[1::2], b.nodes[1::2]) if in_place else (out[0].to_host().view(np.uint8) == 2).all()
    assert lib.allocation_state()[:2] == (4, 640)


@pytest.mark.parametrize("fault", [None, "other handle"] + sorted(FAULTS - {"a caller array is written early", "the unhooked call returns something else"}))
def test_edit_contract(fault):
    lib = Library(fault if fault in FAULTS else None)
    other = Octree(lib, 200)
    base = lib.allocation_state()[:2]
    src = Octree(lib, 100)
    if fault == "other handle":  # src stays whole and is all that is left once dst is empty
        dst, seed, bystanders, left = Octree(lib, 300), 300, [src], (2, 320)
    else:  # in place, as the faults are injected
        dst, seed, bystanders, left, src = src, 100, [other], (0, 0), other
    out = filled(lib, 4, np.uint8)[0]

    def sweep():
        return sweep_edit(lib, lambda: dst.edit(src), dst, lambda: dst.build(seed), base, lambda: dst.listing(src, out), N, bystanders, left)

    if fault in FAULTS:
        with pytest.raises((AssertionError, pytest.fail.Exception)):
            sweep()
        return
    assert sweep() == (N, ADOPT)
    assert np.array_equal(dst.nodes, src.nodes + 1) and lib.allocation_state()[0] == (6 if fault == "other handle" else 4)
