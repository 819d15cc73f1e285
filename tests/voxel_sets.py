"""What the voxel-set operator tests (tests/test_gpu_<operator>.py, their alloc-failure sweeps and CPU models' tests) share: the grid they build on, the builders,
the generators of voxel sets, the strict comparison of array tuples, the canary arrays and the one check that two handles hold the same octree.
tests/test_voxel_sets_cpu.py drives that check with fake handles and sees each of its clauses fire."""
import numpy as np

LOWER, DPS = np.array([-0.3, 0.7, 1.1], np.float32), np.float32(0.013)  # no power of two: products and sums really round
CAGE = [(0, 1, 1), (2, 1, 1), (1, 0, 1), (1, 2, 1), (1, 1, 0), (1, 1, 2)]  # the six face neighbours of (1, 1, 1)


# ---- builders ------------------------------------------------------------------------------------------------------------------------------------------------------
def colours(n, seed=1, emission=True):
    at = np.random.default_rng(seed).integers(0, 256, size=(n, 8), dtype=np.uint8)
    if not emission:
        at[:, 4:7] = 0
    return at


def build(mv, xyz, res, flags=0, attribs=None, seed=1, origin=LOWER, dps=DPS):
    """a fresh handle over xyz; attribs None: colours(len(xyz), seed)"""
    xyz = np.ascontiguousarray(xyz, np.uint32).reshape(-1, 3)
    svo = mv.IntersectorOctreeGPU()
    svo.build_voxels(xyz, colours(len(xyz), seed) if attribs is None else attribs, origin=origin, dps=dps, gridRes=res, flags=flags)
    return svo


def octree(svo):
    return svo.download(want_morton=True)


# ---- generators ----------------------------------------------------------------------------------------------------------------------------------------------------
def full(res):
    return np.stack(np.meshgrid(*[np.arange(res)] * 3, indexing="ij"), -1).reshape(-1, 3)


def shell(lo, hi):
    """the voxels of the hollow cube [lo, hi)^3 (or of the box given by two triples), one voxel thick"""
    lo, hi = np.broadcast_to(lo, 3), np.broadcast_to(hi, 3)
    p = np.stack(np.meshgrid(*[np.arange(a, b) for a, b in zip(lo, hi)], indexing="ij"), -1).reshape(-1, 3)
    return p[((p == lo) | (p == hi - 1)).any(1)]


def holed_shell():
    g = np.zeros((16, 16, 16), bool)
    g[4:11, 4:11, 4:11] = True
    g[5:10, 5:10, 5:10] = False
    g[7, 7, 10] = False
    return np.argwhere(g)


def cavities():
    """(xyz, gridRes) of the sets the models of the nearest voxel are held to the band model on"""
    # (gridRes 8: the band model walks the 137 000 offsets of the largest ball over the whole grid)
    rng = np.random.default_rng(11)
    inner = np.stack(np.meshgrid(*[np.arange(1, 7)] * 3, indexing="ij"), -1).reshape(-1, 3)
    yield np.concatenate([shell(0, 8), inner[rng.random(len(inner)) < 0.04]]), 8  # debris in a cavity, the shell on the grid border
    yield np.concatenate([shell(0, 8), shell(2, 6)]), 8  # nested


def specks_and_block(holes, seed=77):
    """a 12^3 block with one-voxel holes among specks (2 % of a 32^3 grid), unsorted"""
    rng = np.random.default_rng(seed)
    solid = np.ones((12, 12, 12), bool)
    for h in holes:
        solid[h] = False
    return np.concatenate([np.argwhere(rng.random((32, 32, 32)) < 0.02), np.argwhere(solid) + 9])


def block_and_noise(seed, res):
    """(xyz, attribs) of a 12^3 block in 3 % noise on a res^3 grid: what the alloc-failure sweeps of the operators build"""
    rng = np.random.default_rng(seed)
    solid = np.zeros((res, res, res), bool)
    solid[8:20, 8:20, 8:20] = True
    solid |= rng.random((res, res, res)) < 0.03
    xyz = np.argwhere(solid).astype(np.uint32)
    return xyz, rng.integers(0, 256, (len(xyz), 8), dtype=np.uint8)


def tube():
    """a hollow 3 x 3 tube along x, 300 long, closed at both ends, in gridRes 512: one gap of 298 cells whose four neighbour rows hold 298 voxels each"""
    return shell((100, 10, 20), (400, 13, 23))


def serpentine(res=32):
    """a one-cell corridor through a solid res^3 block filling the grid: rows along x at odd y of the odd z layers, joined at alternating ends, the layers joined
    behind the last row of each.  -> (solid (res, res, res) bool, the corridor's cells in walking order)"""
    solid = np.ones((res,) * 3, bool)
    path, right = [], True
    ys = list(range(1, res - 1, 2))
    for z in range(1, res - 1, 2):
        for y in ys:
            xs = range(1, res - 1) if right else range(res - 2, 0, -1)
            path += [(x, y, z) for x in xs]
            right = not right
            if y != ys[-1]:
                path.append((path[-1][0], y + (1 if ys[0] < ys[-1] else -1), z))
        if z + 2 < res - 1:
            path.append((path[-1][0], path[-1][1], z + 1))
        ys.reverse()
    p = np.array(path)
    assert len({tuple(c) for c in path}) == len(path) and (np.abs(np.diff(p, axis=0)).sum(1) == 1).all()
    solid[p[:, 0], p[:, 1], p[:, 2]] = False
    return solid, p


def filler(count, z, res=32):
    """`count` voxels of layer z without an enclosed gap: full rows along x, then a partial row whose last voxel stands at the far border (one exterior gap)"""
    i = np.arange(count)
    p = np.stack([i % res, i // res, np.full(count, z)], 1)
    if 1 < count % res < res - 1:
        p[-1, 0] = res - 1
    return p


# ---- comparisons ---------------------------------------------------------------------------------------------------------------------------------------------------
def same(a, b):
    """two tuples of arrays: as many, and each pair equal in shape and value"""
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def filled(mv, shape, dtype):
    """(device array, host copy) of the canary byte 0x5A"""
    host = np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, 0x5A, np.uint8).view(dtype).reshape(shape)
    return mv.DeviceArray.from_host(host), host


VIEW_MEMBERS = ("cellBlocks", "cellBits", "rootIndex", "rootMask")  # (cellBlocks: a device address, compared as present or absent)


def assert_same_octree(a, b, skip=()):
    """Two handles hold the same octree: every field of the info, the downloaded arrays with the codes, the voxel list, the device view and the resident derived
    tables.  skip: names of info fields that a call site has a stated reason not to compare.  Every assert names what differed: pytest does not rewrite the
    asserts of a helper module."""
    ia, ib = a.info(), b.info()
    for f, _ in ia._fields_:
        if f in skip:
            continue
        x, y = getattr(ia, f), getattr(ib, f)
        x, y = (x[:], y[:]) if hasattr(x, "__len__") else (x, y)
        assert x == y, "info.%s: %r != %r" % (f, x, y)
    for what, x, y in (("download", octree(a), octree(b)), ("read_voxels", a.read_voxels(), b.read_voxels())):
        assert same(x, y), "%s(): %s" % (what, "%d arrays != %d" % (len(x), len(y)) if len(x) != len(y) else ", ".join(
            "[%d] differs, shapes %s and %s" % (i, np.shape(p), np.shape(q)) for i, (p, q) in enumerate(zip(x, y)) if not np.array_equal(p, q)))
    if ia.flavour != 2 and ia.levels <= 16:  # (the tree flavour has no device view, nor have more than 16 levels)
        va, vb = a.device_view(), b.device_view()
        for m in VIEW_MEMBERS:
            x, y = getattr(va, m), getattr(vb, m)
            x, y = (x != 0, y != 0) if m == "cellBlocks" else (x, y)
            assert x == y, "device_view().%s: %r != %r" % (m, x, y)
    assert a.traversal_bytes() == b.traversal_bytes(), "traversal_bytes(): %r != %r" % (a.traversal_bytes(), b.traversal_bytes())  # the resident derived tables
