"""The C calls behind the Python mirror's voxel wrappers, pinned without a library: `massivevoxelraytracing_amd._lib` is replaced by a fake that logs every
call, hands out distinct device addresses and writes scripted counts through the byref arguments.  For every listing: the sizing call carries capacity 0 and
no outputs, the allocations follow it with the right byte sizes in the right order, the filling call carries the counts and exactly those addresses in the
right positions (and is made at a count of 0 only where the wrapper makes it: the surface listings, components, nearest_voxels), and the result has the
right keys, shapes and dtypes.  For every in-place operation: the one call, its arguments and the order of the counts it returns.

Three entries make xyz (36 bytes), attribs (24), uint32 (12), uint8 (3) and uint64 (24 = attribs, but never in one call) differ, so a swapped pointer shows."""
import ctypes as C

import numpy as np
import pytest

import massivevoxelraytracing_amd as mv

H, HB, S = 0xBEEF, 0xB0B, 0x57  # this handle, the second set's handle, the stream: passed through as they are
U64, U32 = "&" + C.c_uint64.__name__, "&" + C.c_uint32.__name__
XF, INFO, HOST = "&CellTransform", "&SvoInfo", "host"
BASE, STEP = 0x100000, 0x1000  # fake device addresses, in allocation order
VOXELS = 7
u8, u16, u32, u64, f32 = np.uint8, np.uint16, np.uint32, np.uint64, np.float32

ENTRIES = ("mvrt_malloc mvrt_free mvrt_memcpy_h2d mvrt_memcpy_d2h mvrt_svo_get_info mvrt_svo_read_voxels mvrt_svo_walk_voxels mvrt_svo_rebuild "
           "mvrt_svo_enclosed_cells mvrt_svo_fill_enclosed mvrt_svo_enclosed_nearest mvrt_svo_fill_enclosed_nearest mvrt_svo_coarse_voxels mvrt_svo_coarsen "
           "mvrt_svo_dilation_cells mvrt_svo_erosion_voxels mvrt_svo_dilate mvrt_svo_erode mvrt_svo_close mvrt_svo_open mvrt_svo_distance_cells "
           "mvrt_svo_depth_voxels mvrt_svo_dilate_ball mvrt_svo_erode_ball mvrt_svo_close_ball mvrt_svo_open_ball mvrt_svo_components mvrt_svo_keep_components "
           "mvrt_svo_combine_voxels mvrt_svo_combine mvrt_svo_nearest_voxels mvrt_svo_nearest_between mvrt_svo_transfer_attributes mvrt_svo_resample_voxels "
           "mvrt_svo_resample mvrt_svo_surface_masks mvrt_svo_surface_exterior_masks mvrt_svo_surface_quads mvrt_svo_surface_quads_masked mvrt_svo_surface_mesh "
           "mvrt_svo_surface_mesh_masked mvrt_svo_surface_merged mvrt_svo_surface_merged_masked mvrt_svo_surface_ao").split()


class FakeLib:
    """one logging function per C entry the voxel wrappers use; every one returns 0"""

    def __init__(self, script, voxels=VOXELS):
        self.log, self.frees, self.mallocs, self.script, self.voxels = [], [], [], {k: list(v) for k, v in script.items()}, voxels
        for name in ENTRIES:
            setattr(self, name, self._entry(name))

    def _entry(self, name):
        def call(*args):
            counts = iter(self.script.get(name, ()))
            plain = []
            for a in args:
                o = getattr(a, "_obj", None)
                if o is not None:  # a byref argument
                    if isinstance(o, mv.SvoInfo):
                        o.numberOfVoxels, o.gridRes, o.dps = self.voxels, 16, 0.25
                    elif isinstance(o, C.c_void_p):
                        o.value = BASE + STEP * len(self.mallocs)
                        self.mallocs.append(o.value)
                    elif isinstance(o, (C.c_uint64, C.c_uint32)):
                        o.value = next(counts, 0)
                    plain.append("&" + type(o).__name__)
                else:
                    plain.append(HOST if isinstance(a, C.c_void_p) else a)
            if name == "mvrt_free":
                self.frees.append(args[0])
            elif name == "mvrt_malloc":
                self.log.append((name, args[1]))
            elif name.startswith("mvrt_memcpy"):
                assert args[3] is None
                self.log.append((name, args[1] if name.endswith("d2h") else args[0], args[2]))  # (the device side, bytes)
            else:
                self.log.append((name,) + tuple(plain))
            return 0
        return call


def CAP(i=0):
    return ("cap", i)


def P(key):
    return ("ptr", key)


def resolve(args, caps, addr):
    """the arguments of one call from their template: capacities and output pointers filled in (None, None = the sizing call)"""
    out = []
    for a in args:
        if isinstance(a, tuple) and a[0] == "cap":
            out.append(0 if caps is None else caps[a[1]])
        elif isinstance(a, tuple) and a[0] == "ptr":
            out.append(None if addr is None else addr.get(a[1]))
        else:
            out.append(a)
    return tuple(out)


class Listing:
    """one listing wrapper: `run` calls it, `fn` and `args` are the C call (after the handle, before the stream), `outs` = (key, entries, trailing shape, dtype)
    in allocation order, `counts` = what the C call reports, `caps` = the capacities of the filling call, `fill` = whether it is made, `fetch` = the keys in
    copy-back order (default: allocation order), `before` / `between` = the calls ahead of the sizing call / between it and the allocations, `scalars` = the
    other entries of the result, `nalloc0` = the allocations made before the outputs, `keys` = the keys of the result in order (default: the copy-back order,
    then the scalars)"""

    def __init__(self, run, fn, args, outs, counts, caps, fill, fetch=None, before=(), between=(), scalars=None, nalloc0=0, keys=None):
        self.__dict__.update(locals())

    def expected(self):
        addr, log = {}, list(self.before)
        log.append((self.fn, H) + resolve(self.args, None, None) + (S,))
        log += list(self.between)
        for i, (key, n, trail, dt) in enumerate(self.outs):
            addr[key] = BASE + STEP * (self.nalloc0 + i)
            log.append(("mvrt_malloc", self.nbytes(key)))
        if self.fill:
            log.append((self.fn, H) + resolve(self.args, self.caps, addr) + (S,))
        return addr, log

    def nbytes(self, key):
        n, trail, dt = [o[1:] for o in self.outs if o[0] == key][0]
        return int(n * np.prod(trail, dtype=np.int64)) * np.dtype(dt).itemsize

    def check(self, fake, result, addr, log, tail=()):
        log = log + list(tail) + [("mvrt_memcpy_d2h", addr[k], self.nbytes(k)) for k in (self.fetch or [o[0] for o in self.outs]) if self.nbytes(k)]
        assert fake.log == log
        if isinstance(result, dict):
            assert list(result) == (self.keys or list(self.fetch or [o[0] for o in self.outs]) + list(self.scalars or {}))
            for key, n, trail, dt in self.outs:
                assert result[key].shape == (n,) + tuple(trail) and result[key].dtype == dt, key
            for k, v in (self.scalars or {}).items():
                assert result[k] == v and type(result[k]) is int, k
        assert sorted(fake.frees) == sorted(fake.mallocs)  # every block is given back when the wrapper returns


def xf():
    return mv.CellTransform.make([1 << 24, 0, 0, 0, 1 << 24, 0, 0, 0, 1 << 24], [0, 0, 0])


def simple(n):
    """the listings of one count: sizing call, allocations, the filling call only where n != 0"""
    X, A, W, B = ("xyz", n, (3,), u32), ("attribs", n, (8,), u8), lambda k: (k, n, (), u32), lambda k: (k, n, (), u8)
    one = dict(caps=(n,), fill=n != 0)
    return {
        "walk_voxels": Listing(lambda s, b: s.walk_voxels(S), "mvrt_svo_walk_voxels", [CAP(), P("xyz"), P("vIndex"), P("attribs"), U64], [X, W("vIndex"), A], [n], **one),
        "enclosed_cells": Listing(lambda s, b: s.enclosed_cells(S), "mvrt_svo_enclosed_cells", [CAP(), P("xyz"), P("region"), U64, U64], [X, W("region")], [n, 5],
                                  scalars={"nRegions": 5}, **one),
        "enclosed_nearest": Listing(lambda s, b: s.enclosed_nearest(S), "mvrt_svo_enclosed_nearest",
                                    [CAP(), P("xyz"), P("region"), P("dist2"), P("nearest"), P("attribs"), U64, U64], [X, W("region"), W("dist2"), W("nearest"), A], [n, 5],
                                    scalars={"nRegions": 5}, **one),
        "coarse_voxels": Listing(lambda s, b: s.coarse_voxels(2, 4, S), "mvrt_svo_coarse_voxels", [2, 4, CAP(), P("xyz"), P("attribs"), P("count"), U64], [X, A, W("count")], [n], **one),
        "dilation_cells": Listing(lambda s, b: s.dilation_cells(mv.MORPH_FACES, S), "mvrt_svo_dilation_cells", [0, CAP(), P("xyz"), P("attribs"), P("count"), U64],
                                  [X, A, W("count")], [n], **one),
        "erosion_voxels": Listing(lambda s, b: s.erosion_voxels(mv.MORPH_FACES, S), "mvrt_svo_erosion_voxels", [0, CAP(), P("vIndex"), U64], [W("vIndex")], [n], **one),
        "distance_cells": Listing(lambda s, b: s.distance_cells(9, S), "mvrt_svo_distance_cells", [9, CAP(), P("xyz"), P("dist2"), P("nearest"), P("attribs"), U64],
                                  [X, W("dist2"), W("nearest"), A], [n], **one),
        "depth_voxels": Listing(lambda s, b: s.depth_voxels(9, S), "mvrt_svo_depth_voxels", [9, CAP(), P("vIndex"), P("depth2"), U64], [W("vIndex"), W("depth2")], [n], **one),
        "combine_voxels": Listing(lambda s, b: s.combine_voxels(b, mv.COMBINE_XOR, (1, 2, 3), mv.COMBINE_ATTRIB_B, S), "mvrt_svo_combine_voxels",
                                  [HB, 3, HOST, 1, CAP(), P("xyz"), P("attribs"), P("source"), U64, U64, U64], [X, A, B("source")], [n, 11, 12],
                                  scalars={"overlap": 11, "clipped": 12}, **one),
        "combine_voxels_no_offset": Listing(lambda s, b: s.combine_voxels(b, mv.COMBINE_UNION, stream=S), "mvrt_svo_combine_voxels",
                                            [HB, 0, None, 0, CAP(), P("xyz"), P("attribs"), P("source"), U64, U64, U64], [X, A, B("source")], [n, 11, 12],
                                            scalars={"overlap": 11, "clipped": 12}, **one),
        "resample_voxels": Listing(lambda s, b: s.resample_voxels(xf(), 8, S), "mvrt_svo_resample_voxels", [XF, 8, CAP(), P("xyz"), P("attribs"), P("source"), U64],
                                   [X, A, W("source")], [n], **one),
    }


def run(case, masks=None):
    """the wrapper under the fake library -> (fake, result); masks: "numpy" / "device" = the masks= keyword in that form"""
    fake = FakeLib({case.fn: case.counts})
    mv._lib = fake  # (monkeypatch has saved the real value)
    s, b = mv.IntersectorOctreeGPU(_borrowed=H), mv.IntersectorOctreeGPU(_borrowed=HB)
    if masks == "device":
        m = mv.DeviceArray(VOXELS, u8)
        del fake.log[:]
        result = case.run(s, b, m)
        del m
    elif masks == "numpy":
        result = case.run(s, b, np.arange(VOXELS, dtype=u8))
    else:
        result = case.run(s, b)
    return fake, result


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    monkeypatch.setattr(mv, "_lib", None)


@pytest.mark.parametrize("n", [0, 3])
@pytest.mark.parametrize("name", sorted(simple(0)))
def test_listing_of_one_count(name, n):
    case = simple(n)[name]
    fake, result = run(case)
    addr, log = case.expected()
    case.check(fake, result, addr, log)
    if name == "erosion_voxels":
        assert result.shape == (n,) and result.dtype == u32


def test_resample_voxels_takes_the_grid_of_the_handle():
    """gridRes None: one info call ahead of each of the two C calls"""
    fake, result = run(Listing(lambda s, b: s.resample_voxels(xf(), None, S), "mvrt_svo_resample_voxels", [], [], [3], (3,), True))
    names = [e[0] for e in fake.log]
    assert names[:2] == ["mvrt_svo_get_info", "mvrt_svo_resample_voxels"] and names[5:7] == ["mvrt_svo_get_info", "mvrt_svo_resample_voxels"]
    assert fake.log[1][3:5] == (16, 0) and fake.log[6][3:5] == (16, 3)


@pytest.mark.parametrize("n", [0, 2])
def test_components(n):
    """label is sized by numberOfVoxels, read between the sizing call and the allocations; the filling call is made at n = 0 too"""
    W = lambda k, m, t=(): (k, m, t, u32)
    case = Listing(lambda s, b: s.components(mv.MORPH_FACES, S), "mvrt_svo_components", [0, P("label"), CAP(), P("size"), P("first"), P("box"), U64, U64],
                   [W("label", VOXELS), W("size", n), W("first", n), W("box", n, (6,))], [n, 4], (n,), True, between=[("mvrt_svo_get_info", H, INFO)])
    fake, result = run(case)
    addr, log = case.expected()
    assert [e[1] for e in log if e[0] == "mvrt_malloc"] == [28, 4 * n, 4 * n, 24 * n]
    case.check(fake, result, addr, log)
    fake, both = run(Listing(lambda s, b: s.components_device(mv.MORPH_CUBE, 1, 2, 3, 4, 5, S), "mvrt_svo_components", [], [], [n, 4], (n,), True))
    assert fake.log == [("mvrt_svo_components", H, 1, 1, 2, 3, 4, 5, U64, U64, S)] and both == (n, 4)


def masked(masks):
    """what masks= adds: (the calls ahead of the sizing call, the leading argument of the masked entry, allocations made before the outputs)"""
    if masks is None:
        return [], [], 0
    if masks == "numpy":
        return [("mvrt_malloc", VOXELS), ("mvrt_memcpy_h2d", BASE, VOXELS)], [BASE], 1
    return [], [BASE], 1


MASKS = [None, "numpy", "device"]


@pytest.mark.parametrize("masks", MASKS)
@pytest.mark.parametrize("n", [0, 3])
def test_surface_quads(n, masks):
    before, lead, k = masked(masks)
    case = Listing(lambda s, b, m=None: s.surface_quads(S, masks=m), "mvrt_svo_surface_quads" + ("_masked" if masks else ""),
                   lead + [CAP(), P("faceVoxel"), P("faceDir"), P("positions"), U64], [("faceVoxel", n, (), u32), ("faceDir", n, (), u8), ("positions", n, (4, 3), f32)],
                   [n], (n,), True, before=before, nalloc0=k)
    fake, result = run(case, masks)
    addr, log = case.expected()
    assert [e[1] for e in log if e[0] == "mvrt_malloc"][-3:] == [4 * n, n, 48 * n]
    case.check(fake, result, addr, log)


@pytest.mark.parametrize("masks", MASKS)
@pytest.mark.parametrize("nf,nv", [(0, 0), (3, 5)])
def test_surface_mesh(nf, nv, masks):
    before, lead, k = masked(masks)
    case = Listing(lambda s, b, m=None: s.surface_mesh(S, masks=m), "mvrt_svo_surface_mesh" + ("_masked" if masks else ""),
                   lead + [CAP(0), CAP(1), P("faceVoxel"), P("faceDir"), P("indices"), P("vertices"), U64, U64],
                   [("faceVoxel", nf, (), u32), ("faceDir", nf, (), u8), ("indices", nf, (4,), u32), ("vertices", nv, (3,), f32)], [nf, nv], (nf, nv), True,
                   fetch=["vertices", "indices", "faceVoxel", "faceDir"], before=before, nalloc0=k)
    fake, result = run(case, masks)
    addr, log = case.expected()
    assert [e[1] for e in log if e[0] == "mvrt_malloc"][-4:] == [4 * nf, nf, 16 * nf, 12 * nv]
    case.check(fake, result, addr, log)
    assert list(result) == ["vertices", "indices", "faceVoxel", "faceDir"]


@pytest.mark.parametrize("masks", MASKS)
@pytest.mark.parametrize("weld", [False, True])
@pytest.mark.parametrize("nf,nr,nv", [(0, 0, 0), (3, 2, 5)])
def test_surface_merged(nf, nr, nv, weld, masks):
    """without the weld flag indices and vertices are neither allocated nor passed; with it they come after the four rectangle arrays"""
    before, lead, k = masked(masks)
    flags = mv.SURFACE_MERGE_ANY_ATTRIBUTE | (mv.SURFACE_MERGE_WELD if weld else 0)
    outs = [("rectVoxel", nr, (), u32), ("rectDir", nr, (), u8), ("rectSize", nr, (2,), u32), ("positions", nr, (4, 3), f32)]
    fetch = [o[0] for o in outs]
    if weld:
        outs += [("indices", nr, (4,), u32), ("vertices", nv, (3,), f32)]
        fetch += ["vertices", "indices"]
    case = Listing(lambda s, b, m=None: s.surface_merged(flags, S, masks=m), "mvrt_svo_surface_merged" + ("_masked" if masks else ""),
                   lead + [flags, CAP(0), CAP(1), P("rectVoxel"), P("rectDir"), P("rectSize"), P("positions"), P("indices"), P("vertices"), U64, U64, U64], outs, [nf, nr, nv],
                   (nr, nv), True, fetch=fetch, before=before, nalloc0=k, keys=["nFaces"] + fetch)
    fake, result = run(case, masks)
    addr, log = case.expected()
    assert [e[1] for e in log if e[0] == "mvrt_malloc"][k if masks == "numpy" else 0:] == [4 * nr, nr, 8 * nr, 48 * nr] + ([16 * nr, 12 * nv] if weld else [])
    case.check(fake, result, addr, log)
    assert list(result) == ["nFaces"] + fetch and result["nFaces"] == nf


@pytest.mark.parametrize("masks", MASKS)
@pytest.mark.parametrize("n", [0, 3])
def test_surface_ao(n, masks):
    """the faces without their positions, then the occlusion call on them, both at n = 0 too"""
    before, lead, k = masked(masks)
    case = Listing(lambda s, b, m=None: s.surface_ao(4, 0.5, S, masks=m), "mvrt_svo_surface_quads" + ("_masked" if masks else ""),
                   lead + [CAP(), P("faceVoxel"), P("faceDir"), P("positions"), U64], [("faceVoxel", n, (), u32), ("faceDir", n, (), u8), ("open", n, (), u16)],
                   [n], (n,), True, before=before, nalloc0=k)
    fake, result = run(case, masks)
    addr, log = case.expected()
    assert [e[1] for e in log if e[0] == "mvrt_malloc"][-3:] == [4 * n, n, 2 * n]
    case.check(fake, result, addr, log, tail=[("mvrt_svo_surface_ao", H, n, addr["faceVoxel"], addr["faceDir"], 4, 0.5, addr["open"], S)])
    fake, result = run(Listing(lambda s, b: s.surface_ao(stream=S), "mvrt_svo_surface_quads", [], [], [n], (n,), True))
    assert fake.log[0] == ("mvrt_svo_get_info", H, INFO) and [e for e in fake.log if e[0] == "mvrt_svo_surface_ao"][0][5:7] == (64, 2.0)  # radius = 8 * dps


@pytest.mark.parametrize("call,fn,counts", [("surface_masks", "mvrt_svo_surface_masks", [9]), ("surface_exterior_masks", "mvrt_svo_surface_exterior_masks", [9, 2])])
def test_masks_listings(call, fn, counts):
    """sized by numberOfVoxels: info, one allocation, the one call, the copy back"""
    fake, result = run(Listing(lambda s, b: getattr(s, call)(S), fn, [], [], counts, (), True))
    assert fake.log == [("mvrt_svo_get_info", H, INFO), ("mvrt_malloc", VOXELS), (fn, H, BASE) + (U64,) * len(counts) + (S,), ("mvrt_memcpy_d2h", BASE, VOXELS)]
    assert result[0].shape == (VOXELS,) and result[0].dtype == u8 and list(result[1:]) == counts
    fake, result = run(Listing(lambda s, b: getattr(s, call + "_device")(None, S), fn, [], [], counts, (), True))
    assert fake.log == [(fn, H, None) + (U64,) * len(counts) + (S,)] and result == (counts[0] if len(counts) == 1 else tuple(counts))


def test_read_voxels():
    fake, (xyz, attribs) = run(Listing(lambda s, b: s.read_voxels(S), "mvrt_svo_read_voxels", [], [], [], (), True))
    assert fake.log == [("mvrt_svo_get_info", H, INFO), ("mvrt_malloc", 12 * VOXELS), ("mvrt_malloc", 8 * VOXELS), ("mvrt_svo_read_voxels", H, BASE, BASE + STEP, S),
                        ("mvrt_memcpy_d2h", BASE, 12 * VOXELS), ("mvrt_memcpy_d2h", BASE + STEP, 8 * VOXELS)]
    assert (xyz.shape, xyz.dtype, attribs.shape, attribs.dtype) == ((VOXELS, 3), u32, (VOXELS, 8), u8)


@pytest.mark.parametrize("n", [0, 3])
def test_nearest_voxels(n):
    """the call with no query first, then the queries and the outputs; the second call is made for no query too"""
    fn = "mvrt_svo_nearest_voxels"
    fake, result = run(Listing(lambda s, b: s.nearest_voxels(np.arange(3 * n, dtype=np.int32).reshape(n, 3), 50, S), fn, [], [], [], (), True))
    q, d, v, a = [BASE + STEP * i for i in range(4)]
    assert fake.log == ([(fn, H, 0, None, 50, None, None, None, S), ("mvrt_malloc", 12 * n)] + ([("mvrt_memcpy_h2d", q, 12 * n)] if n else []) +
                        [("mvrt_malloc", 8 * n), ("mvrt_malloc", 4 * n), ("mvrt_malloc", 8 * n), (fn, H, n, q, 50, d, v, a, S)] +
                        ([("mvrt_memcpy_d2h", d, 8 * n), ("mvrt_memcpy_d2h", v, 4 * n), ("mvrt_memcpy_d2h", a, 8 * n)] if n else []))
    assert list(result) == ["dist2", "nearest", "attribs"]
    assert [(result[k].shape, result[k].dtype) for k in result] == [((n,), u64), ((n,), u32), ((n, 8), u8)]
    fake = FakeLib({})
    mv._lib = fake
    with pytest.raises(ValueError, match="outside"):
        mv.IntersectorOctreeGPU(_borrowed=H).nearest_voxels([[0, 0, (1 << 22) + 1]])
    assert fake.log == []  # refused before any C call


@pytest.mark.parametrize("n", [0, 3])
def test_nearest_between(n):
    """sized by numberOfVoxels, no sizing call; an empty handle gets the summary call alone.  farthest, the uint32, is the third counter of the C call"""
    fn = "mvrt_svo_nearest_between"
    fake = FakeLib({fn: [n, 40, 6, 1, 2]}, voxels=n)
    mv._lib = fake
    r = mv.IntersectorOctreeGPU(_borrowed=H).nearest_between(mv.IntersectorOctreeGPU(_borrowed=HB), (1, 2, 3), 50, S)
    counters = (U64, U64, U32, U64, U64, S)
    if n == 0:
        assert fake.log == [("mvrt_svo_get_info", H, INFO), (fn, H, HB, HOST, 50, 0, None, None) + counters]
        assert list(r) == ["n", "maxDist2", "farthest", "zero", "beyond"]
    else:
        assert fake.log == [("mvrt_svo_get_info", H, INFO), ("mvrt_malloc", 8 * n), ("mvrt_malloc", 4 * n), (fn, H, HB, HOST, 50, n, BASE, BASE + STEP) + counters,
                            ("mvrt_memcpy_d2h", BASE, 8 * n), ("mvrt_memcpy_d2h", BASE + STEP, 4 * n)]
        assert list(r) == ["n", "maxDist2", "farthest", "zero", "beyond", "dist2", "nearest"]
        assert (r["dist2"].shape, r["dist2"].dtype, r["nearest"].shape, r["nearest"].dtype) == ((n,), u64, (n,), u32)
    assert [r[k] for k in ("n", "maxDist2", "farthest", "zero", "beyond")] == [n, 40, 6, 1, 2]
    assert sorted(fake.frees) == sorted(fake.mallocs)


IN_PLACE = {
    # name: (call, C entry, its arguments between handle and stream, scripted counts, the wrapper's result)
    "fill_enclosed": (lambda s, b: s.fill_enclosed(None, S), "mvrt_svo_fill_enclosed", (None, U64), [3], 3),
    "fill_enclosed_attrib": (lambda s, b: s.fill_enclosed(np.arange(8, dtype=u8), S), "mvrt_svo_fill_enclosed", (HOST, U64), [3], 3),
    "fill_enclosed_nearest": (lambda s, b: s.fill_enclosed_nearest(S), "mvrt_svo_fill_enclosed_nearest", (U64,), [3], 3),
    "dilate": (lambda s, b: s.dilate(mv.MORPH_FACES, 2, S), "mvrt_svo_dilate", (0, 2, U64), [3], 3),
    "erode": (lambda s, b: s.erode(mv.MORPH_FACES, 2, S), "mvrt_svo_erode", (0, 2, U64), [3], 3),
    "close": (lambda s, b: s.close(mv.MORPH_CUBE, 2, S), "mvrt_svo_close", (1, 2, U64), [3], 3),
    "open": (lambda s, b: s.open(stream=S), "mvrt_svo_open", (1, 1, U64), [3], 3),
    "dilate_ball": (lambda s, b: s.dilate_ball(9, S), "mvrt_svo_dilate_ball", (9, U64), [3], 3),
    "erode_ball": (lambda s, b: s.erode_ball(9, S), "mvrt_svo_erode_ball", (9, U64), [3], 3),
    "close_ball": (lambda s, b: s.close_ball(9, S), "mvrt_svo_close_ball", (9, U64), [3], 3),
    "open_ball": (lambda s, b: s.open_ball(stream=S), "mvrt_svo_open_ball", (1, U64), [3], 3),
    "keep_components": (lambda s, b: s.keep_components(mv.MORPH_FACES, 4, 2, S), "mvrt_svo_keep_components", (0, 4, 2, U64, U64), [3, 5], (3, 5)),
    "combine": (lambda s, b: s.combine(b, mv.COMBINE_DIFFERENCE, (1, 2, 3), 1, S), "mvrt_svo_combine", (HB, 2, HOST, 1, U64, U64, U64), [3, 5, 7], (3, 5, 7)),
    "transfer_attributes": (lambda s, b: s.transfer_attributes(b, None, 50, mv.TRANSFER_COLOUR, S), "mvrt_svo_transfer_attributes", (HB, None, 50, 1, U64, U64), [3, 5], (3, 5)),
    "resample": (lambda s, b: s.resample(xf(), b, (0, 0, 0), 0.5, 8, 1, S)._h, "mvrt_svo_resample", (HB, XF, HOST, 0.5, 8, 1, U64), [3], HB),
    "coarsen": (lambda s, b: s.coarsen(2, 4, 1, b, S)._h, "mvrt_svo_coarsen", (HB, 2, 4, 1), [], HB),
    "rebuild": (lambda s, b: s.rebuild(1, S), "mvrt_svo_rebuild", (1,), [], None),
}


@pytest.mark.parametrize("name", sorted(IN_PLACE))
def test_in_place(name):
    call, fn, args, counts, want = IN_PLACE[name]
    fake, result = run(Listing(call, fn, [], [], counts, (), True))
    assert fake.log == [(fn, H) + args + (S,)] and result == want


def test_resample_in_place_takes_its_own_lattice():
    fake, result = run(Listing(lambda s, b: s.resample(xf(), stream=S)._h, "mvrt_svo_resample", [], [], [3], (), True))
    assert fake.log == [("mvrt_svo_get_info", H, INFO), ("mvrt_svo_resample", H, H, XF, HOST, 0.25, 16, 0, U64, S)] and result == H


DEVICE_FORMS = {
    # the *_device forms with every argument given: (call, C entry, arguments between handle and stream, counts, result)
    "walk_voxels_device": (lambda s, b: s.walk_voxels_device(9, 1, 2, 3, S), "mvrt_svo_walk_voxels", (9, 1, 2, 3, U64), [3], 3),
    "enclosed_cells_device": (lambda s, b: s.enclosed_cells_device(9, 1, 2, S), "mvrt_svo_enclosed_cells", (9, 1, 2, U64, U64), [3, 5], (3, 5)),
    "enclosed_nearest_device": (lambda s, b: s.enclosed_nearest_device(9, 1, 2, 3, 4, 5, S), "mvrt_svo_enclosed_nearest", (9, 1, 2, 3, 4, 5, U64, U64), [3, 5], (3, 5)),
    "combine_voxels_device": (lambda s, b: s.combine_voxels_device(b, 1, None, 0, 9, 1, 2, 3, S), "mvrt_svo_combine_voxels", (HB, 1, None, 0, 9, 1, 2, 3, U64, U64, U64), [3, 5, 7],
                              (3, 5, 7)),
    "surface_mesh_device": (lambda s, b: s.surface_mesh_device(9, 8, 1, 2, 3, 4, S), "mvrt_svo_surface_mesh", (9, 8, 1, 2, 3, 4, U64, U64), [3, 5], (3, 5)),
    "surface_merged_device": (lambda s, b: s.surface_merged_device(2, 9, 8, 1, 2, 3, 4, 5, 6, S), "mvrt_svo_surface_merged", (2, 9, 8, 1, 2, 3, 4, 5, 6, U64, U64, U64), [3, 2, 5],
                              (3, 2, 5)),
    "surface_merged_device_masked": (lambda s, b: s.surface_merged_device(2, 9, 8, 1, 2, 3, 4, 5, 6, S, masks=7), "mvrt_svo_surface_merged_masked",
                                     (7, 2, 9, 8, 1, 2, 3, 4, 5, 6, U64, U64, U64), [3, 2, 5], (3, 2, 5)),
    "nearest_between_device": (lambda s, b: s.nearest_between_device(b, None, 50, 9, 1, 2, S), "mvrt_svo_nearest_between", (HB, None, 50, 9, 1, 2, U64, U64, U32, U64, U64),
                               [3, 40, 6, 1, 2], {"n": 3, "maxDist2": 40, "farthest": 6, "zero": 1, "beyond": 2}),
    "surface_ao_device": (lambda s, b: s.surface_ao_device(3, 1, 2, 4, 0.5, 3, S), "mvrt_svo_surface_ao", (3, 1, 2, 4, 0.5, 3), [], None),
}


@pytest.mark.parametrize("name", sorted(DEVICE_FORMS))
def test_device_forms_pass_pointers_through(name):
    """the order of the counts in a multi-count return, and raw device pointers passed on as given"""
    call, fn, args, counts, want = DEVICE_FORMS[name]
    fake, result = run(Listing(call, fn, [], [], counts, (), True))
    assert fake.log == [(fn, H) + args + (S,)] and result == want


def test_voxel_arrays_refusals_come_before_any_call():
    fake = FakeLib({})
    mv._lib = fake
    s = mv.IntersectorOctreeGPU(_borrowed=H)
    with pytest.raises(ValueError, match="xyz must be"):
        s.edit_voxels(0x1234)
    assert fake.log == []
    with pytest.raises(ValueError, match="ops has 2 entries, xyz 3"):
        s.edit_voxels(np.zeros((3, 3), u32), None, np.zeros(2, u8))
