"""Merged surface on the GPU (mvrt_svo_surface_merged) against the numpy model of tests/merge_expected.py: counts, rectVoxel, rectDir, rectSize, positions,
vertices and indices bit for bit, on the smallest inputs that can break each mechanism -- hand cases, tiny random grids with two attribute values, launch and
scan seams, runs and stacks across many workgroups, the row wrap of the packed keys (every gridRes, and the 21-bit edge), attributes, edits, flavours -- and
the contract of the call (capacities, NULL outputs, refusals).  The model's attributes are the library's own read_voxels bytes.  The weld limit
(4 * nRects >= 2^32) is a host comparison in surfaceMerged (csrc/kernels_surface.hip) and is covered by reading: reaching it takes 2^30 rectangles."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import common
import merge_expected as M
import surface_expected as S
from common import bunny_tris
from fixtures import mv  # noqa: F401 (fixtures)
from voxel_sets import DPS, LOWER, filled, full

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_FLAGS = (0, M.ANY_ATTRIBUTE, M.WELD, M.ANY_ATTRIBUTE | M.WELD)
RED, BLUE = (200, 10, 10, 255, 0, 0, 0, 255), (10, 10, 200, 255, 0, 0, 0, 255)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def build(mv, xyz, res, attrs=None, flags=0):
    svo = mv.IntersectorOctreeGPU()
    svo.build_voxels(np.ascontiguousarray(xyz, np.uint32), None if attrs is None else np.ascontiguousarray(attrs, np.uint8), origin=LOWER, dps=DPS, gridRes=res, flags=flags)
    return svo


def assert_merged(svo, res, flags_list=ALL_FLAGS, lower=LOWER, dps=DPS):
    """the call of `svo` == the model on the handle's own voxel list, for each of `flags_list`; the two model-free invariants; -> {flags: model dict}"""
    xyz, attrs = svo.read_voxels()
    xyz = xyz.astype(np.int64)
    masks, n_faces = svo.surface_masks()
    quads = None
    out = {}
    for flags in flags_list:
        want = M.merged(xyz, attrs, res, lower, dps, flags)
        got = svo.surface_merged(flags)
        n = len(want["rectVoxel"])
        assert got["nFaces"] == want["nFaces"] == n_faces
        assert svo.surface_merged_device(flags) == (n_faces, n, len(want["vertices"]) if flags & M.WELD else 0)  # the sizing call
        assert np.array_equal(got["rectVoxel"], want["rectVoxel"]) and np.array_equal(got["rectDir"], want["rectDir"]), flags
        assert got["rectSize"].shape == (n, 2) and np.array_equal(got["rectSize"], want["rectSize"]), flags
        assert got["positions"].shape == (n, 4, 3) and np.array_equal(bits(got["positions"]), bits(want["positions"])), flags
        if flags & M.WELD:
            assert np.array_equal(got["indices"], want["indices"]) and np.array_equal(bits(got["vertices"]), bits(want["vertices"])), flags
        else:
            assert "indices" not in got and "vertices" not in got
        # whatever the model says: the rectangles cover nFaces faces, and exactly those of surface_quads, none twice
        assert int(got["rectSize"].astype(np.int64).prod(1).sum()) == n_faces
        if quads is None:
            q = svo.surface_quads()
            quads = np.concatenate([xyz[q["faceVoxel"]], q["faceDir"][:, None].astype(np.int64)], 1)
        assert M.same_face_set(M.rasterise(xyz, got["rectVoxel"], got["rectDir"], got["rectSize"]), quads), flags
        out[flags] = want
    return out


def check(mv, xyz, res, attrs=None, flags_list=ALL_FLAGS, build_flags=0):
    svo = build(mv, xyz, res, attrs, build_flags)
    return svo, assert_merged(svo, res, flags_list)


def two_colours(rng, n):
    return np.array([RED, BLUE], np.uint8)[rng.integers(0, 2, size=n)]


# ---- hand cases ---------------------------------------------------------------------------------------------------------------------------------------------
def test_one_voxel_is_six_unit_rectangles(mv):
    svo, want = check(mv, [(2, 3, 5)], 8)
    q = svo.surface_quads()
    m = svo.surface_merged()
    assert m["rectSize"].tolist() == [[1, 1]] * 6 and np.array_equal(m["rectVoxel"], q["faceVoxel"]) and np.array_equal(m["rectDir"], q["faceDir"])
    assert np.array_equal(bits(m["positions"]), bits(q["positions"]))  # the bits and the winding of surface_quads
    w, mesh = svo.surface_merged(M.WELD), svo.surface_mesh()
    assert np.array_equal(w["indices"], mesh["indices"]) and np.array_equal(bits(w["vertices"]), bits(mesh["vertices"]))


@pytest.mark.parametrize("res", [2, 4, 8])
def test_full_grid_is_six_squares(mv, res):
    _, want = check(mv, full(res), res)
    assert want[0]["rectSize"].tolist() == [[res, res]] * 6 and len(want[M.WELD]["vertices"]) == 8


def test_the_L_gives_ten_rectangles(mv):
    _, want = check(mv, [(0, 0, 0), (1, 0, 0), (2, 0, 0), (0, 0, 1), (1, 0, 1)], 4)
    assert want[0]["nFaces"] == 20 and len(want[0]["rectVoxel"]) == 10  # (the count of surface_masks; tests/test_surface_merge_cpu.py walks through the ten)


def test_pair_at_the_upper_edge_merges(mv):
    _, want = check(mv, [(14, 9, 9), (15, 9, 9)], 16)
    assert [tuple(s) for s in want[0]["rectSize"].tolist()] == [(2, 1), (2, 1), (2, 1), (1, 1), (2, 1), (1, 1)]


# ---- random fill ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("density", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("res", [4, 8, 16])
def test_random_fill(mv, res, density):
    rng = np.random.default_rng(2000 * res + int(density * 10))
    xyz = np.argwhere(rng.random((res, res, res)) < density)
    border = [(0, 1, 2), (res - 1, 2, 1), (1, 0, 2), (2, res - 1, 1), (2, 1, 0), (1, 2, res - 1)]  # all six grid borders
    xyz = S.sorted_voxels(np.concatenate([xyz, border]))
    svo, want = check(mv, xyz, res, two_colours(rng, len(xyz)))
    attrs = svo.read_voxels()[1]
    assert len(np.unique(attrs.view(np.uint64))) == 2 and np.all(attrs[:, 3] == 255)  # both colours arrived, alpha as the build stores it
    assert len(want[0]["rectVoxel"]) >= len(want[M.ANY_ATTRIBUTE]["rectVoxel"])


# ---- launch and scan seams ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513, 4097])
def test_voxel_counts(mv, n):
    """the first n cells of a 64^3 grid in Morton order, in two colours"""
    rng = np.random.default_rng(n)
    check(mv, S.decode(np.arange(n, dtype=np.uint64)), 64, two_colours(rng, n), flags_list=(0, M.ANY_ATTRIBUTE | M.WELD))


@pytest.mark.parametrize("axis", [0, 2])
def test_bar_across_many_workgroups(mv, axis):
    """1024 voxels in a line at gridRes 1024.  Along x: for +-Y and +-Z one run of 1024 faces over four workgroups of the head kernel.  Along z: for +-X and
    +-Y (v = z) a stack of 1024 runs of one face"""
    xyz = np.full((1024, 3), 7)
    xyz[:, axis] = np.arange(1024)
    _, want = check(mv, xyz, 1024, flags_list=(0, M.WELD))
    assert len(want[0]["rectVoxel"]) == 6 and want[0]["nFaces"] == 4 * 1024 + 2 and len(want[M.WELD]["vertices"]) == 8
    long_side = (1024, 1) if axis == 0 else (1, 1024)
    sizes = [tuple(s) for s in want[0]["rectSize"].tolist()]
    assert sizes.count((1, 1)) == 2 and sizes.count(long_side) + sizes.count(long_side[::-1]) == 4 and sizes.count(long_side) >= 2


def test_slab_is_one_rectangle_above_and_one_below(mv):
    x, z = np.meshgrid(np.arange(300), np.arange(300), indexing="ij")
    xyz = np.stack([x.reshape(-1) + 3, np.full(90000, 5), z.reshape(-1) + 11], -1)
    _, want = check(mv, xyz, 512, flags_list=(M.WELD,))
    w = want[M.WELD]
    assert w["rectSize"][w["rectDir"] <= 1].tolist() == [[300, 300]] * 2 and len(w["rectVoxel"]) == 6 and len(w["vertices"]) == 8


# ---- the row wrap: keys are packed at `levels` bits per field, so a row's last face and the next row's first differ by 1 at EVERY gridRes ------------------
def sparse_set(res, seed, n=3000):
    rng = np.random.default_rng(seed)
    xyz = rng.integers(0, res, size=(n, 3))
    near = xyz[:600].copy()  # adjacent pairs along every axis
    near[np.arange(600), np.arange(600) % 3] += np.where(near[np.arange(600), np.arange(600) % 3] < res - 1, 1, -1)
    return np.concatenate([xyz, near])


@pytest.mark.parametrize("res", [4, 8, 1 << 21])
def test_row_wrap_pair_stays_unmerged(mv, res):
    y, z = (1, 1) if res <= 8 else (5, 7)
    e = res - 1
    pairs = [(e, y, z), (0, y, z + 1)]  # +-Y: (u, v) = (x, z), step 1
    cols = [(2, 2, e), (2, 3, 0)] if res > 4 else []  # +-X: (u, v) = (y, z), step 2; at gridRes 4 the set below has it
    more = [(e - 1, e, e), (e, e, e)]  # merges: a 2 x 1 at the far corner of the grid
    rng = np.random.default_rng(res % 1000)
    if res > 8:
        xyz = np.concatenate([sparse_set(res, 3), pairs, cols, more])  # a few thousand loose voxels: the masks come from the search path
        attrs = two_colours(rng, len(xyz))
        attrs[-6:] = RED
    else:
        xyz, attrs = np.array(pairs + cols + more), None
    svo, want = check(mv, xyz, res, attrs)
    if res > 8:
        assert svo.info().levels == 21  # above 14 levels a build keeps no cell index (the device view, which would show it, stops at 16 levels)
    got = svo.surface_merged(M.ANY_ATTRIBUTE)
    v = {tuple(p): i for i, p in enumerate(svo.read_voxels()[0].tolist())}
    for a, b in [pairs] + ([cols] if cols else []):
        for i in (v[a], v[b]):  # all six faces of both voxels stay 1 x 1
            assert got["rectSize"][got["rectVoxel"] == i].tolist() == [[1, 1]] * 6, (a, b)
    far = got["rectSize"][got["rectVoxel"] == v[more[0]]].tolist()
    assert far.count([2, 1]) == 4 and len(far) == 5


def test_column_wrap_at_grid_of_four(mv):
    """step 2 at gridRes 4: for +-X (u, v) = (y, z), the runs at (u = 1, v = 3) and (u = 2, v = 0) are neighbours in the packed key only"""
    svo, want = check(mv, [(2, 1, 3), (2, 2, 0)], 4)
    assert want[0]["rectSize"].tolist() == [[1, 1]] * 12


# ---- attributes -------------------------------------------------------------------------------------------------------------------------------------------------
def test_emission_alone_splits(mv):
    xyz = S.sorted_voxels([(x, 2, 2) for x in range(1, 7)])
    attrs = np.tile(np.array(RED, np.uint8), (6, 1))
    attrs[3:, 4:7] = (0, 9, 0)  # the same colour, another emission
    svo, want = check(mv, xyz, 8, attrs)
    got = svo.read_voxels()[1]
    assert len(np.unique(got[:, :4].copy().view(np.uint32))) == 1 and len(np.unique(got[:, 4:].copy().view(np.uint32))) == 2
    assert len(want[0]["rectVoxel"]) == 2 + 4 * 2 and len(want[M.ANY_ATTRIBUTE]["rectVoxel"]) == 6


def test_alpha_byte_alone_splits(mv):
    """builds and edits store alpha 255; an upload keeps its bytes and a rebuild copies them verbatim"""
    xyz = S.sorted_voxels([(x, y, 2) for x in range(1, 7) for y in (3, 4)])
    src = build(mv, xyz, 8, np.tile(np.array(RED, np.uint8), (12, 1)))
    nodes, attrs, _ = src.download()
    i = src.info()
    for byte in (3, 7):
        changed = attrs.copy().reshape(-1, 8)
        changed[::2, byte] = 17
        up = mv.IntersectorOctreeGPU()
        up.upload(nodes, changed, LOWER, DPS, 8, i.hasEmission, embeddedMask=bool(i.embeddedMask))
        up.rebuild()
        assert np.array_equal(up.read_voxels()[1], changed)
        want = assert_merged(up, 8)
        assert len(want[0]["rectVoxel"]) > len(want[M.ANY_ATTRIBUTE]["rectVoxel"]) == 6
    assert len(assert_merged(src, 8, (0,))[0]["rectVoxel"]) == 6  # without the byte: six rectangles


def test_edits(mv):
    rng = np.random.default_rng(8)
    old = S.sorted_voxels(np.concatenate([np.argwhere(rng.random((32, 32, 32)) < 0.3), [(15, 9, 9), (16, 9, 9)]]))
    svo, before = check(mv, old, 32, np.tile(np.array(RED, np.uint8), (len(old), 1)))
    quads = svo.surface_quads()
    # attribute-only: the faces stay, the rectangles change
    svo.edit_voxels(old[::3].astype(np.uint32), np.tile(np.array(BLUE, np.uint8), (len(old[::3]), 1)))
    after = assert_merged(svo, 32)
    q2 = svo.surface_quads()
    assert all(np.array_equal(quads[k], q2[k]) for k in quads)
    assert len(after[0]["rectVoxel"]) > len(before[0]["rectVoxel"])
    assert np.array_equal(after[M.ANY_ATTRIBUTE]["rectSize"], before[M.ANY_ATTRIBUTE]["rectSize"])
    # structural, across the seam x = 15 | 16 of the cell index's blocks: a row of 8 through it, and one voxel of the old pair removed
    row = np.array([(x, 20, 20) for x in range(12, 20)])
    svo.edit_voxels(np.concatenate([row, [(16, 9, 9)]]).astype(np.uint32), np.tile(np.array(BLUE, np.uint8), (9, 1)), np.array([1] * 8 + [0], np.uint8))
    assert svo.info().numberOfVoxels == len({tuple(p) for p in old.tolist()} | {tuple(p) for p in row.tolist()}) - 1
    assert_merged(svo, 32)


# ---- flavours -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_tree_flavour_gives_identical_bytes(mv):
    rng = np.random.default_rng(5)
    xyz = S.sorted_voxels(np.argwhere(rng.random((64, 64, 64)) < 0.03))
    attrs = two_colours(rng, len(xyz))
    a, tree = build(mv, xyz, 64, attrs), build(mv, xyz, 64, attrs, flags=3)
    assert tree.info().flavour == 2 and a.device_view().cellBlocks != 0
    assert_merged(a, 64, (M.WELD,))
    x, y = a.surface_merged(M.WELD), tree.surface_merged(M.WELD)
    assert all(np.array_equal(np.ascontiguousarray(x[k]).view(np.uint8), np.ascontiguousarray(y[k]).view(np.uint8)) for k in x if k != "nFaces") and x["nFaces"] == y["nFaces"]


def test_triangle_build(mv):
    tris = bunny_tris()
    v = tris.reshape(-1, 3)
    lo = v.min(0)
    dps = np.float32((v.max(0) - lo).max() / np.float32(64))
    svo = mv.IntersectorOctreeGPU()
    svo.build(v, None, None, None, lo, dps, 64)
    want = assert_merged(svo, 64, (0, M.WELD), lo, dps)
    assert len(want[0]["rectVoxel"]) < want[0]["nFaces"]


# ---- the contract of the call -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(mv):
    rng = np.random.default_rng(12)
    xyz = S.sorted_voxels(np.argwhere(rng.random((16, 16, 16)) < 0.3))
    attrs = two_colours(rng, len(xyz))
    svo = build(mv, xyz, 16, attrs)
    return svo, M.merged(xyz, attrs, 16, LOWER, DPS, M.WELD)


def test_capacity_one_short(mv, small):
    svo, want = small
    f, n, m = want["nFaces"], len(want["rectVoxel"]), len(want["vertices"])
    outs = {k: filled(mv, s, t) for k, s, t in (("rv", n, np.uint32), ("rd", n, np.uint8), ("rs", (n, 2), np.uint32), ("pos", (n, 12), np.float32), ("idx", (n, 4), np.uint32),
                                                ("vtx", (m, 3), np.float32))}
    p = {k: v[0].ptr for k, v in outs.items()}
    lib = mv.lib()
    nf, nr, nv = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    for caps, what, count in (((n - 1, m), b"rectCapacity %d" % (n - 1), b"%d rectangles" % n), ((n, m - 1), b"vertexCapacity %d" % (m - 1), b"%d vertices" % m)):
        nf.value = nr.value = nv.value = 0
        assert lib.mvrt_svo_surface_merged(svo._h, M.WELD, caps[0], caps[1], p["rv"], p["rd"], p["rs"], p["pos"], p["idx"], p["vtx"], C.byref(nf), C.byref(nr), C.byref(nv), None) != 0
        assert (nf.value, nr.value, nv.value) == (f, n, m) and what in lib.mvrt_last_error() and count in lib.mvrt_last_error()
    assert lib.mvrt_svo_surface_merged(svo._h, 0, n - 1, 0, p["rv"], None, None, None, None, None, C.byref(nf), C.byref(nr), C.byref(nv), None) != 0
    assert (nf.value, nr.value, nv.value) == (f, n, 0) and b"rectCapacity" in lib.mvrt_last_error()
    for dev, host in outs.values():
        assert np.array_equal(dev.to_host().view(np.uint8), host.view(np.uint8))  # nothing was written
    with pytest.raises(mv.MvrtError, match="rectCapacity"):
        svo.surface_merged_device(0, n - 1, 0, outs["rv"][0])
    # a larger capacity than the count is fine and writes the count's worth
    assert svo.surface_merged_device(0, n + 7, 0, mv.DeviceArray(n + 7, np.uint32)) == (f, n, 0)


def test_each_output_alone(mv, small):
    svo, want = small
    f, n, m = want["nFaces"], len(want["rectVoxel"]), len(want["vertices"])
    assert svo.surface_merged_device() == (f, n, 0) and svo.surface_merged_device(M.WELD) == (f, n, m)  # sizing calls: capacities 0, all NULL
    shapes = {"rectVoxel": (n, np.uint32), "rectDir": (n, np.uint8), "rectSize": ((n, 2), np.uint32), "positions": ((n, 4, 3), np.float32), "indices": ((n, 4), np.uint32),
              "vertices": ((m, 3), np.float32)}
    for name, (shape, dtype) in shapes.items():
        dev = mv.DeviceArray(shape, dtype)
        caps = (0, m) if name == "vertices" else (n, 0)  # the capacity of what is not asked for is not looked at
        flags = M.WELD if name in ("indices", "vertices") else 0
        assert svo.surface_merged_device(flags, caps[0], caps[1], **{name: dev}) == (f, n, m if flags else 0)
        assert np.array_equal(np.ascontiguousarray(dev.to_host()).view(np.uint8), np.ascontiguousarray(want[name]).view(np.uint8)), name
    assert mv.lib().mvrt_svo_surface_merged(svo._h, 0, 0, 0, None, None, None, None, None, None, None, None, None, None) == 0  # even the counts may be NULL


def test_positions_at_an_odd_address(mv, small):
    """a positions array that is not 16-byte aligned takes the scalar stores"""
    svo, want = small
    n = len(want["rectVoxel"])
    buf = mv.DeviceArray(n * 12 + 1, np.float32)
    svo.surface_merged_device(0, n, 0, positions=buf.ptr + 4)
    assert np.array_equal(bits(buf.to_host()[1:]), bits(want["positions"]).reshape(-1))


def test_refusals_without_gpu_work(mv, small):
    svo, want = small
    n = len(want["rectVoxel"])
    empty = mv.IntersectorOctreeGPU()
    nodes, attrs, _ = svo.download()
    i = svo.info()
    up = mv.IntersectorOctreeGPU()
    up.upload(nodes, attrs, LOWER, DPS, 16, i.hasEmission, embeddedMask=bool(i.embeddedMask))
    idx, vtx = filled(mv, (n, 4), np.uint32), filled(mv, (len(want["vertices"]), 3), np.float32)
    before = mv.allocation_state()[2]
    for h, text in ((empty, "no octree"), (up, "keeps no Morton codes")):
        for flags in ALL_FLAGS:
            with pytest.raises(mv.MvrtError, match=text):
                h.surface_merged_device(flags)
    for flags in (4, 8, 0x80000003):
        with pytest.raises(mv.MvrtError, match="unknown flags"):
            svo.surface_merged_device(flags)
    for flags in (0, M.ANY_ATTRIBUTE):  # indices or vertices without the weld flag
        for kw in ({"indices": idx[0]}, {"vertices": vtx[0]}):
            with pytest.raises(mv.MvrtError, match="MVRT_SURFACE_MERGE_WELD"):
                svo.surface_merged_device(flags, n, len(want["vertices"]), **kw)
    nv = C.c_uint64(77)
    assert mv.lib().mvrt_svo_surface_merged(svo._h, 0, n, 0, None, None, None, None, idx[0].ptr, None, None, None, C.byref(nv), None) != 0 and nv.value == 0
    assert mv.allocation_state()[2] == before
    for dev, host in (idx, vtx):
        assert np.array_equal(dev.to_host().view(np.uint8), host.view(np.uint8))


def test_the_handle_is_not_modified(mv, small):
    svo, want = small
    before = svo.download(want_morton=True)
    held = mv.allocation_state()[:2]
    assert_merged(svo, 16)
    assert all(np.array_equal(a, b) for a, b in zip(svo.download(want_morton=True), before))
    assert mv.allocation_state()[:2] == held  # the scratch is gone


# ---- upper layers ---------------------------------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_runs(tmp_path, mv):
    exe, libdir = common.compile_usage(tmp_path, "surface_merge_usage")
    out = subprocess.check_output([str(exe), "run"], timeout=120).decode()
    assert "faces 24 rects 6 vertices 8 sized 24 6 8 same 1 two 1" in out


@pytest.mark.parametrize("weld", [True, False])
@pytest.mark.parametrize("option,any_attribute", [("--merge", 0), ("--merge-any", M.ANY_ATTRIBUTE)])
def test_voxel_mesh_app(tmp_path, mv, option, any_attribute, weld):
    from massivevoxelraytracing_amd import build as b
    b.build_apps(verbose=False)
    tris = bunny_tris()
    v = tris.reshape(-1, 3)
    with open(tmp_path / "bunny.obj", "w") as f:
        f.write("".join("v %.9g %.9g %.9g\n" % tuple(p) for p in v) + "".join("f %d %d %d\n" % (3 * t + 1, 3 * t + 2, 3 * t + 3) for t in range(len(tris))))
    out = subprocess.check_output([os.path.join(ROOT, "apps", "voxel_mesh"), str(tmp_path / "bunny.obj"), "64", str(tmp_path / "bunny.ply"), option] + ([] if weld else ["--no-weld"]),
                                  timeout=120).decode()
    lo = v.min(0)
    svo = mv.IntersectorOctreeGPU()
    svo.build(v, None, None, None, lo, np.float32((v.max(0) - lo).max() / np.float32(64)), 64)
    vertices, indices, colours = S.read_ply_quads(tmp_path / "bunny.ply")
    _, attrs = svo.read_voxels()
    m = svo.surface_merged(any_attribute | (M.WELD if weld else 0))
    if weld:
        assert np.array_equal(bits(vertices), bits(m["vertices"])) and np.array_equal(indices, m["indices"])
    else:
        assert np.array_equal(bits(vertices), bits(m["positions"].reshape(-1, 3))) and np.array_equal(indices.reshape(-1), np.arange(len(indices) * 4))
    assert np.array_equal(colours, attrs[m["rectVoxel"], :3])
    assert out.strip().splitlines()[-1].split("->")[0].strip().endswith("faces %d rects %d vertices %d" % (m["nFaces"], len(indices), len(vertices)))
