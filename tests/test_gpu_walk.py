"""mvrt_svo_walk_voxels and mvrt_svo_rebuild on the GPU against the numpy model of tests/walk_expected.py, the oracle's builder and the library's own
read-back, integers and bytes bit for bit.  The scenes are the smallest that reach each way the walk can go wrong: a root whose children are voxels (no
frontier level), one-voxel chains, the empty octree, several thousand parents with uneven child counts (offsets across the 256-parent groups), a 63-bit
prefix at 21 levels; every legal upload shape of tests/upload_shapes.py, both flavours; hand-made trees whose last frontier is 255, 256 and 257 parents, and
one with a whole group of 256 childless parents between two groups with children."""
import os
import subprocess

import numpy as np
import pytest

import common
import deep_scenes as D
import surface_expected as S
import upload_shapes as U
import walk_expected as W
from common import hdr_bytes, probe_camera
from edit_model import assert_svo, has_emission, normalised, oracle_octree
from fixtures import mv, O  # noqa: F401 (fixtures)
from rays import random_rays
from upload_shapes import Base, bases, oracle_scene, shapes, upload  # noqa: F401 (bases is a fixture)
from voxel_sets import filled

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXF = np.float32(3.402823466e38)
SCENES = ["single1", "single2", "single3", "empty", "random7", "random9", "bunny256", "deep14", "deep21"]


@pytest.fixture(scope="module")
def scenes(O, bases):
    out = dict(bases)
    s = D.DeepScene(21)
    sc = D.oracle_scene(O, s)
    out["deep21"] = Base("deep21", sc.morton, sc.attrs, s.res, s.origin, s.dps, sc.has_emission)
    return out


_shapes = {}


def shapes_of(O, scenes, scene, emb):
    """(base, {shape: nodes}, {shape: model}) -- generated once per scene and flavour, never changed"""
    key = (scene, emb)
    if key not in _shapes:
        base = None if scene == "empty" else scenes[scene]
        nodes = {k: v[0] for k, v in shapes(O, base, emb, 11 + len(scene)).items()}
        res = 4 if base is None else base.res
        _shapes[key] = (base, nodes, {k: W.walk(n, res, emb) for k, n in nodes.items()})
    return _shapes[key]


def assert_walk(got, want_xyz, want_vi, want_attrs):
    assert np.array_equal(got["xyz"], want_xyz) and got["xyz"].dtype == np.uint32
    assert np.array_equal(got["vIndex"], want_vi)
    assert np.array_equal(got["attribs"], want_attrs)


# ---- 1. the walk of every legal shape ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("emb", [True, False])
@pytest.mark.parametrize("scene", SCENES)
def test_walk_of_every_legal_shape(mv, O, scenes, scene, emb):
    base, nodes, model = shapes_of(O, scenes, scene, emb)
    for name, nd in nodes.items():
        sc = oracle_scene(O, base, nd, emb)
        svo = upload(mv, sc, emb)
        paths, vi, xyz = model[name]
        n = len(paths)
        assert svo.walk_voxels_device() == n, name  # the sizing call
        assert_walk(svo.walk_voxels(), xyz, vi, sc.attrs[vi])
        assert np.array_equal(svo.download()[0].view(O.NODE_DTYPE), nd), name  # the handle is not modified
        if n == 0:
            assert scene == "empty"
            assert svo.walk_voxels_device(0, mv.DeviceArray(1, np.uint32)) == 0  # an output and nothing to write: succeeds
    # the contract of the call, on the last shape ("all"; the empty octree has nothing to write)
    if n == 0:
        return
    dx, dv, da = mv.DeviceArray((n, 3), np.uint32), mv.DeviceArray(n, np.uint32), mv.DeviceArray((n, 8), np.uint8)
    assert svo.walk_voxels_device(n, dx, None, None) == n and np.array_equal(dx.to_host(), xyz)  # each output alone
    assert svo.walk_voxels_device(n, None, dv, None) == n and np.array_equal(dv.to_host(), vi)
    assert svo.walk_voxels_device(n + 5, None, None, da) == n and np.array_equal(da.to_host(), sc.attrs[vi])  # a larger capacity writes the count's worth
    outs = [filled(mv, (n, 3), np.uint32), filled(mv, n, np.uint32), filled(mv, (n, 8), np.uint8)]
    import ctypes as C
    cnt = C.c_uint64(0)
    lib = mv.lib()
    assert lib.mvrt_svo_walk_voxels(svo._h, n - 1, outs[0][0].ptr, outs[1][0].ptr, outs[2][0].ptr, C.byref(cnt), None) != 0
    assert cnt.value == n and b"capacity %d" % (n - 1) in lib.mvrt_last_error() and b"%d voxels" % n in lib.mvrt_last_error()
    for dev, host in outs:
        assert np.array_equal(dev.to_host().view(np.uint8), host.view(np.uint8))  # nothing was written
    assert lib.mvrt_svo_walk_voxels(svo._h, 0, None, None, None, None, None) == 0  # even the count may be NULL


# ---- 2. a built handle ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("scene", ["single1", "random7", "deep21"])
def test_built_handle_walks_like_read_voxels(mv, scenes, scene, flags):
    base = scenes[scene]
    svo = mv.IntersectorOctreeGPU()
    svo.build_voxels(D.decode(base.morton), base.attrs, origin=base.origin, dps=base.dps, gridRes=base.res, flags=flags)
    info = svo.info()
    assert info.flavour == {0: 0, 1: 0, 2: 1, 3: 2}[flags]  # embedded, embedded (no DAG), plain, tree
    xyz, attrs = svo.read_voxels()
    n = len(xyz)
    assert n == len(base.morton)
    assert_walk(svo.walk_voxels(), xyz, np.arange(n), attrs)  # answered from the codes
    # the forced walk: the same octree through download and upload keeps no codes and is walked from the root -- the same bytes
    nodes, dattrs, _ = svo.download()
    up = mv.IntersectorOctreeGPU()
    up.upload(nodes, dattrs, base.origin, base.dps, base.res, info.hasEmission, embeddedMask=bool(info.embeddedMask))
    with pytest.raises(mv.MvrtError, match="keeps no Morton codes"):
        up.read_voxels()
    assert_walk(up.walk_voxels(), xyz, np.arange(n), attrs)


# ---- 3. rebuild -------------------------------------------------------------------------------------------------------------------------------------------
REBUILDS = [("random7", "all", 0), ("random7", "psum_random", 1), ("random7", "empty_inner", 2), ("random7", "psum_zero", 0), ("single1", "builder", 0), ("single2", "permute", 1),
            ("bunny256", "unshare", 0), ("deep14", "all", 2), ("deep21", "unreachable", 0)]


@pytest.mark.parametrize("emb", [True, False])
@pytest.mark.parametrize("scene,shape,flags", REBUILDS)
def test_rebuild_makes_the_octree_of_a_voxel_list_build(mv, O, scenes, scene, shape, flags, emb):
    base, nodes, model = shapes_of(O, scenes, scene, emb)
    paths, vi, xyz = model[shape]
    n = len(paths)
    sc = oracle_scene(O, base, nodes[shape], emb)
    for he in ((sc.has_emission, 0) if base.attrs[:, 4:7].any() else (sc.has_emission,)):  # also an upload that says "no emission" over emissive attributes
        svo = mv.IntersectorOctreeGPU()
        svo.upload(sc.nodes, sc.attrs, sc.origin, sc.dps, sc.grid_res, he, embeddedMask=emb)
        svo.set_emission_scale(3.25)
        before = svo.info()
        svo.rebuild(flags)
        want_attrs = sc.attrs[vi]  # verbatim, in Morton-rank order
        assert_svo(O, svo, paths, want_attrs, he, base.res, flags, n)
        info = svo.info()
        assert (info.gridRes, info.dps, info.emissionScale) == (before.gridRes, before.dps, before.emissionScale)
        assert list(info.lower) == list(before.lower) and list(info.upper) == list(before.upper)
        rx, ra = svo.read_voxels()
        assert np.array_equal(rx, xyz) and np.array_equal(ra, want_attrs)
        assert_walk(svo.walk_voxels(), xyz, np.arange(n), want_attrs)
    want = S.surface(xyz, base.res, sc.origin, sc.dps)
    masks, nf = svo.surface_masks()
    assert np.array_equal(masks, want["masks"]) and nf == want["nFaces"]
    if base.res <= 512 and n > 1:  # (deeper grids: the index is an accelerator the library drops when memory is short)
        assert svo.device_view().cellBlocks != 0  # the cell index exists now
    # one edit: a removal, a re-colouring and an insertion; the build flags of the rebuild are kept
    d = {int(k): a for k, a in zip(paths, want_attrs)}
    free = next(c for c in range(base.res ** 3) if c not in d)
    exyz = D.decode(np.array([paths[0], paths[-1], free], np.uint64))
    eattrs = np.array([[0] * 8, [1, 2, 3, 4, 5, 6, 7, 8], [9, 8, 7, 6, 0, 0, 0, 5]], np.uint8)
    svo.edit_voxels(exyz, eattrs, np.array([0, 1, 1], np.uint8))
    d.pop(int(paths[0]))
    d[int(paths[-1])], d[free] = normalised(eattrs[1])[0], normalised(eattrs[2])[0]
    m = np.array(sorted(d), np.uint64)
    a = np.array([d[int(k)] for k in m], np.uint8).reshape(-1, 8)
    assert_svo(O, svo, m, a, has_emission(a), base.res, flags, 0)


# ---- 4. the same picture ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("emb", [True, False])
@pytest.mark.parametrize("scene,shape", [("random7", "psum_random"), ("bunny256", "all")])
def test_rebuild_keeps_the_picture(mv, O, scenes, scene, shape, emb):
    base, nodes, model = shapes_of(O, scenes, scene, emb)
    paths, vi, _ = model[shape]
    sc = oracle_scene(O, base, nodes[shape], emb)
    ro, rd = random_rays(sc, 20_000, 77)
    # the rank of the path a ray hits: what the oracle reports on the builder's octree of the same voxels (nVoxelsPSum sums = Morton ranks)
    rank = oracle_scene(O, base, O.build_octree(paths, base.res, embed=emb), emb).trace(ro, rd, None, threads=min(16, len(os.sched_getaffinity(0))))
    rgba, hw, hh = O.decode_rgbe(hdr_bytes())
    pt = mv.PathTracer()
    pt.setup(None)
    pt.resizeFrameBufferIfNeeded(None, 96, 54)
    pt.loadHDRIPixels(None, rgba, hw, hh, rgba, hw, hh)
    svo = upload(mv, sc, emb, pt.m_intersectorOctreeGPU)
    cam = probe_camera(sc.origin, sc.dps, sc.grid_res, focus=9.0, lens_r=0.05, offset=(1.5, 1.0, 1.5) if scene != "bunny256" else (6, 4, 6))
    b = svo.intersect(ro, rd)
    attrs_before = svo.download()[1]
    pt.step(None, cam)
    fb = pt.read_framebuffer()
    assert fb[:, :3].any()
    svo.rebuild(0)  # through the path tracer's intersector: the step in flight finishes first
    pt.clearFrameBuffer()
    pt.step(None, cam)
    assert np.array_equal(pt.read_framebuffer().view(np.uint32), fb.view(np.uint32))
    a = svo.intersect(ro, rd)
    attrs_after = svo.download()[1]
    hit = b["t"] != MAXF
    assert hit.sum() > 2000
    assert np.array_equal(a["t"], b["t"]) and np.array_equal(a["nMajor"], b["nMajor"])
    assert np.array_equal(attrs_before[b["vIndex"][hit]], attrs_after[a["vIndex"][hit]])
    assert np.array_equal(a["vIndex"][hit], rank["vIndex"][hit]) and np.array_equal(rank["t"], a["t"])
    assert shape != "psum_random" or (a["vIndex"][hit] != b["vIndex"][hit]).sum() > 1000  # the numbering really changed, the picture did not
    del pt


# ---- 5. refusals leave the handle as it was ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_as_it_was(mv, O, scenes):
    none = mv.IntersectorOctreeGPU()
    before = mv.allocation_state()[2]
    for call in (none.walk_voxels_device, none.walk_voxels, none.rebuild):
        with pytest.raises(mv.MvrtError, match="no octree"):
            call()
    assert mv.allocation_state()[2] == before and none.info().numberOfNodes == 0
    for emb in (True, False):
        empty = upload(mv, oracle_scene(O, None, shapes(O, None, emb, 0)["empty"][0], emb), emb)
        with pytest.raises(mv.MvrtError, match="holds no voxel"):
            empty.rebuild()
        assert empty.info().numberOfNodes == 1 and empty.walk_voxels_device() == 0
        base, nodes, model = shapes_of(O, scenes, "random7", emb)
        sc = oracle_scene(O, base, nodes["all"], emb)
        svo = upload(mv, sc, emb)
        ro, rd = random_rays(sc, 6000, 5)
        want = svo.intersect(ro, rd, want_descents=True)
        info = bytes(svo.info())
        for flags in (4, 8, -1, 1 << 20):
            with pytest.raises(mv.MvrtError, match="unsupported flags"):
                svo.rebuild(flags)
            got = svo.intersect(ro, rd, want_descents=True)
            assert all(np.array_equal(got[k], want[k]) for k in want) and bytes(svo.info()) == info
        assert np.array_equal(svo.download()[0].view(O.NODE_DTYPE), nodes["all"])
        with pytest.raises(mv.MvrtError, match="keeps no Morton codes"):
            svo.read_voxels()  # a plain upload is still refused: nothing walks implicitly
        with pytest.raises(mv.MvrtError, match="keeps no Morton codes"):
            svo.surface_masks_device()
        with pytest.raises(mv.MvrtError, match="keeps no Morton codes"):
            svo.edit_voxels(np.zeros((1, 3), np.uint32))


# ---- 6. a change of flavour -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first,then", [(0, 1), (0, 2), (0, 3), (3, 0), (1, 0)])
def test_rebuild_of_a_built_handle_changes_the_flavour(mv, O, scenes, first, then):
    base = scenes["random7"]
    svo = mv.IntersectorOctreeGPU()
    svo.build_voxels(D.decode(base.morton), base.attrs, origin=base.origin, dps=base.dps, gridRes=base.res, flags=first)
    attrs = normalised(base.attrs)
    assert_svo(O, svo, base.morton, attrs, base.he, base.res, first, len(base.morton))
    svo.rebuild(then)
    assert_svo(O, svo, base.morton, attrs, base.he, base.res, then, len(base.morton), nodes=oracle_octree(O, base.morton, base.res, then))
    assert svo.info().flavour == {0: 0, 1: 0, 2: 1, 3: 2}[then]
    assert_walk(svo.walk_voxels(), D.decode(base.morton), np.arange(len(base.morton)), attrs)


# ---- 7. the seams of the emit kernel's groups -----------------------------------------------------------------------------------------------------------
def tree_of(O, leaf_masks, levels, emb):
    """The octree (a tree: no sharing, children numbered before their parent, root last, the builder's nVoxelsPSum) whose parents of voxels are the keys of
    leaf_masks -- paths of levels - 1 octal digits -- with the given masks of voxels.  Mask 0 is a reachable empty node, legal in an upload."""
    prefixes = {(levels - 1 - up, k >> (3 * up)) for k in leaf_masks for up in range(levels)}  # (depth, path so far)
    rows = []

    def make(prefix, depth):  # -> (index, own mask, voxels below)
        kids, psum, mask, count = [U.LEAF] * 8, [0] * 8, 0, 0
        for c in range(8):
            psum[c] = count
            if depth == levels - 1:
                if leaf_masks[prefix] >> c & 1:
                    mask, count = mask | 1 << c, count + 1
            elif (depth + 1, prefix * 8 + c) in prefixes:
                i, m, n = make(prefix * 8 + c, depth + 1)
                kids[c], mask, count = (i | m << 24) if emb else i, mask | 1 << c, count + n
        rows.append((mask, kids, psum))
        return len(rows) - 1, mask, count

    n_voxels = make(0, 0)[2]
    nodes = np.zeros(len(rows), O.NODE_DTYPE)
    nodes["mask"], nodes["children"], nodes["psum"] = [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]
    return nodes, n_voxels


def seam_masks(name):
    """-> (levels, {path: mask}) with the parents of voxels in path order cut into the emit kernel's groups of 256 where it can go wrong"""
    rng = np.random.default_rng(len(name))
    if name == "empty_group":  # 770 parents: the whole second group (256 .. 511) has mask 0, between two groups with children
        keys = np.sort(rng.choice(8 ** 4, 770, replace=False))
        masks = rng.integers(1, 256, 770)
        masks[rng.random(770) < 0.2] = 0
        masks[250:515] = 0
        masks[[0, 249, 515, 769]] = [0x81, 0xFF, 0x01, 0x80]
        return 5, dict(zip(keys.tolist(), masks.tolist()))
    n = int(name)  # 255, 256, 257 parents: one group short of full, full, and one parent in a second group
    keys = np.sort(rng.choice(8 ** 3, n, replace=False))
    masks = rng.integers(1, 256, n)
    masks[rng.random(n) < 0.2] = 0
    masks[[0, 254]] = [0x80, 0xFF]  # children in the first and the last full lane of the first group
    masks[n - 1] = 0x01 if n != 256 else 0  # the last parent: one child, or none (the group's run ends before its last item)
    return 4, dict(zip(keys.tolist(), masks.tolist()))


@pytest.mark.parametrize("emb", [True, False])
@pytest.mark.parametrize("name", ["255", "256", "257", "empty_group"])
def test_frontiers_at_the_group_seams(mv, O, name, emb):
    levels, leaf_masks = seam_masks(name)
    res = 1 << levels
    nodes, nv = tree_of(O, leaf_masks, levels, emb)
    U.set_masks_zero_padding(nodes)
    assert mv.IntersectorOctreeGPU.check_upload(nodes, nv, res, emb) is None
    # what the scene is for, from the nodes themselves: the frontier of the last level in path order, and its runs of mask 0
    frontier = nodes["mask"][U.depths(nodes, emb) == levels - 1]  # (a tree numbered in path order: index order is path order)
    assert len(frontier) == len(leaf_masks) and np.array_equal(frontier, [leaf_masks[k] for k in sorted(leaf_masks)])
    if name == "empty_group":
        assert len(frontier) > 512 and not frontier[256:512].any() and frontier[:256].any() and frontier[512:].any()
        zero_run = max(len(r) for r in "".join("0" if m == 0 else "1" for m in frontier).split("1"))
        assert zero_run >= 256
    else:
        assert len(frontier) == int(name)
    rng = np.random.default_rng(5)
    attrs = rng.integers(0, 256, (nv, 8), dtype=np.uint8)
    paths, vi, xyz = W.walk(nodes, res, emb)
    assert len(paths) == nv == int(sum(bin(m).count("1") for m in leaf_masks.values())) and np.array_equal(vi, np.arange(nv))
    svo = mv.IntersectorOctreeGPU()
    svo.upload(nodes, attrs, (0.0, 0.0, 0.0), np.float32(1.0 / res), res, int(attrs[:, 4:7].any()), embeddedMask=emb)
    assert svo.walk_voxels_device() == nv
    assert_walk(svo.walk_voxels(), xyz, vi, attrs[vi])


# ---- upper layers -----------------------------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_runs(tmp_path, mv):
    exe, libdir = common.compile_usage(tmp_path, "walk_usage")
    out = subprocess.check_output([str(exe), "run"], timeout=120).decode()
    assert "paths 4 counted 4 walked 1 voxels 4 emission 1 same 1 faces 24" in out
