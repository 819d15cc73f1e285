"""tests/voxel_sets.py against handles made of Python: assert_same_octree passes two equal handles, and for each of its clauses a pair that differs only there
fails with a message that names the clause (a helper module's asserts are not rewritten by pytest, so the message is all a failure shows).  The tree flavour
and octrees of more than 16 levels have no device view; everything else is still compared.  same() refuses tuples of unequal length."""
import copy
import types

import numpy as np
import pytest

from massivevoxelraytracing_amd import SvoInfo
from voxel_sets import VIEW_MEMBERS, assert_same_octree, same

ARRAYS = ("nodes", "attrs", "morton")
VOXELS = ("xyz", "attribs")


class Handle:
    """the five readers of an IntersectorOctreeGPU that assert_same_octree calls"""

    def __init__(self):
        self._info = SvoInfo(numberOfNodes=9, numberOfVoxels=4, lower=(-0.3, 0.7, 1.1), upper=(0.7, 1.7, 2.1), dps=0.25, emissionScale=2.0, hasEmission=1, embeddedMask=1,
                             gridRes=4, levels=2, totalDumpedVoxels=5, flavour=1, reserved=0)
        rng = np.random.default_rng(3)
        self.arrays = {"nodes": rng.integers(0, 2**32, (9, 4), dtype=np.uint32), "attrs": rng.integers(0, 256, (4, 8), dtype=np.uint8),
                       "morton": np.arange(4, dtype=np.uint64), "xyz": rng.integers(0, 4, (4, 3), dtype=np.uint32), "attribs": rng.integers(0, 256, (4, 8), dtype=np.uint8)}
        self.view = types.SimpleNamespace(cellBlocks=0x7F0000001000, cellBits=3, rootIndex=8, rootMask=0x81)
        self.tables = 4096
        self.viewed = 0

    def info(self):
        return self._info

    def download(self, want_morton=False):
        assert want_morton
        return tuple(self.arrays[k] for k in ARRAYS if k in self.arrays)

    def read_voxels(self):
        return tuple(self.arrays[k] for k in VOXELS if k in self.arrays)

    def device_view(self):
        assert self._info.flavour != 2 and self._info.levels <= 16, "no device view"
        self.viewed += 1
        return self.view

    def traversal_bytes(self):
        return self.tables


def pair():
    a = Handle()
    return a, copy.deepcopy(a)


def differs(a, b, clause, **kw):
    with pytest.raises(AssertionError) as e:
        assert_same_octree(a, b, **kw)
    assert clause in str(e.value), (clause, str(e.value))
    with pytest.raises(AssertionError):  # in either order
        assert_same_octree(b, a, **kw)


def test_equal_handles_pass():
    a, b = pair()
    b.view.cellBlocks += 0x1000  # an address: only its presence is compared
    assert_same_octree(a, b)
    assert_same_octree(a, a)
    assert a.viewed == 3 and b.viewed == 1


@pytest.mark.parametrize("field", [f for f, _ in SvoInfo._fields_])
def test_each_info_field(field):
    a, b = pair()
    v = getattr(b._info, field)
    if hasattr(v, "__len__"):
        v[2] += 1  # the last element: the arrays are compared whole
    else:
        setattr(b._info, field, v + 1)
    if field in ("flavour", "levels"):
        b.view = a.view
    differs(a, b, "info." + field)
    if field not in ("flavour", "levels"):
        assert_same_octree(a, b, skip=(field,))  # a site that skips the field compares the rest
        a.tables += 1
        differs(a, b, "traversal_bytes", skip=(field,))


@pytest.mark.parametrize("name", ARRAYS + VOXELS)
def test_each_array_by_value(name):
    a, b = pair()
    b.arrays[name][-1, ...] ^= 1
    what = "download" if name in ARRAYS else "read_voxels"
    differs(a, b, "%s(): [%d]" % (what, (ARRAYS if name in ARRAYS else VOXELS).index(name)))


@pytest.mark.parametrize("name", ARRAYS + VOXELS)
def test_each_array_by_shape(name):
    a, b = pair()
    a.arrays[name], b.arrays[name] = np.zeros(0, a.arrays[name].dtype), np.zeros((0, 3), a.arrays[name].dtype)  # no element differs: only the shape does
    differs(a, b, "shapes (0,) and (0, 3)")


@pytest.mark.parametrize("name", ARRAYS + VOXELS)
def test_each_array_missing(name):
    a, b = pair()
    del b.arrays[name]  # (without the last one, what remains equals a's as far as it goes: a zip would stop there and see nothing)
    differs(a, b, "%s(): %d arrays != %d" % (("download", 3, 2) if name in ARRAYS else ("read_voxels", 2, 1)))


@pytest.mark.parametrize("member", VIEW_MEMBERS)
def test_each_view_member(member):
    a, b = pair()
    setattr(b.view, member, 0 if member == "cellBlocks" else getattr(b.view, member) + 1)
    differs(a, b, "device_view()." + member)


def test_traversal_bytes():
    a, b = pair()
    b.tables += 1
    differs(a, b, "traversal_bytes()")


@pytest.mark.parametrize("field,value", [("flavour", 2), ("levels", 17)])
def test_no_device_view_for_the_tree_flavour_and_beyond_16_levels(field, value):
    a, b = pair()
    for h in (a, b):
        setattr(h._info, field, value)
    b.view.rootMask ^= 1  # (never read)
    assert_same_octree(a, b)
    assert a.viewed == b.viewed == 0
    b._info.reserved = 1
    differs(a, b, "info.reserved")
    b._info.reserved = 0
    b.arrays["morton"][0] += 1
    differs(a, b, "download(): [2]")
    b.arrays["morton"][0] -= 1
    b.arrays["attribs"][0, 0] ^= 1
    differs(a, b, "read_voxels(): [1]")
    b.arrays["attribs"][0, 0] ^= 1
    b.tables += 1
    differs(a, b, "traversal_bytes()")


def test_same_rejects_tuples_of_unequal_length():
    x, y = np.arange(3), np.ones((2, 2))
    assert same((x, y), (x.copy(), y.copy())) and same((), ())
    assert not same((x, y), (x,)) and not same((x,), (x, y)) and not same((), (x,))
    assert not same((x, y), (x, y.reshape(4))) and not same((np.zeros(0),), (np.zeros((0, 3)),))
