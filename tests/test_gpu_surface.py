"""Surface extraction on the GPU (mvrt_svo_surface_masks / _quads / _mesh) against the numpy model of tests/surface_expected.py: masks, counts, faceVoxel,
faceDir, positions, vertices and indices bit for bit, on the smallest inputs that can break each mechanism -- tiny grids, the seams of the cell index's
16-voxel blocks, launch and scan seams, the search path of octrees without a cell index (up to the 21-bit edge), every flavour, edits, and the contract of
the calls (capacities, NULL outputs, refusals).  The weld limit (4 * nFaces >= 2^32) is a host comparison in surfaceMesh (csrc/kernels_surface.hip) and is
covered by reading: reaching it takes a surface of 2^30 faces."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import common
import surface_expected as S
from common import bunny_tris
from fixtures import mv  # noqa: F401 (fixtures)
from voxel_sets import DPS, LOWER, filled, full

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def build(mv, xyz, res, flags=0):
    svo = mv.IntersectorOctreeGPU()
    svo.build_voxels(np.ascontiguousarray(xyz, np.uint32), None, origin=LOWER, dps=DPS, gridRes=res, flags=flags)
    return svo


def assert_surface(svo, want):
    """all three calls of `svo` == the model's dict `want`"""
    masks, n = svo.surface_masks()
    assert np.array_equal(masks, want["masks"]) and n == want["nFaces"]
    assert svo.surface_masks_device(None) == n  # count only
    q = svo.surface_quads()
    assert np.array_equal(q["faceVoxel"], want["faceVoxel"]) and np.array_equal(q["faceDir"], want["faceDir"])
    assert q["positions"].shape == (n, 4, 3) and np.array_equal(bits(q["positions"]), bits(want["positions"]))
    m = svo.surface_mesh()
    assert np.array_equal(m["faceVoxel"], want["faceVoxel"]) and np.array_equal(m["faceDir"], want["faceDir"])
    assert np.array_equal(m["indices"], want["indices"]) and np.array_equal(bits(m["vertices"]), bits(want["vertices"]))


def check(mv, xyz, res, flags=0):
    want = S.surface(xyz, res, LOWER, DPS)
    svo = build(mv, xyz, res, flags)
    assert svo.info().numberOfVoxels == len(want["xyz"])
    assert_surface(svo, want)
    return svo, want


# ---- tiny grids ---------------------------------------------------------------------------------------------------------------------------------------------
def test_grid_of_two(mv):
    """levels = 1: the cell index has no bits inside a block"""
    _, one = check(mv, [(1, 0, 1)], 2)
    assert one["masks"].tolist() == [63]
    _, eight = check(mv, full(2), 2)
    assert eight["nFaces"] == 24 and len(eight["vertices"]) == 26


@pytest.mark.parametrize("res", [4, 8])
def test_full_grid(mv, res):
    _, want = check(mv, full(res), res)
    assert want["nFaces"] == 6 * res * res
    inner = np.all((want["xyz"] > 0) & (want["xyz"] < res - 1), axis=1)
    assert inner.sum() == (res - 2) ** 3 and not want["masks"][inner].any()


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("density", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("res", [4, 8, 16])
def test_random_fill(mv, res, density, seed):
    rng = np.random.default_rng(1000 * res + 10 * int(density * 10) + seed)
    xyz = np.argwhere(rng.random((res, res, res)) < density)
    border = [(0, 1, 2), (res - 1, 2, 1), (1, 0, 2), (2, res - 1, 1), (2, 1, 0), (1, 2, res - 1)]  # all six grid borders
    check(mv, np.concatenate([xyz, border]), res)


# ---- the seams of the cell index: blocks of 8 x 8 x 8 cells = 16 voxels per edge ----------------------------------------------------------------------------
def seam_set(res):
    v = []
    for s in ([15] if res == 32 else [15, 31]):  # pairs straddling s | s + 1 on every axis, in blocks that both hold voxels
        v += [(s, 3, 3), (s + 1, 3, 3), (3, s, 3), (3, s + 1, 3), (3, 3, s), (3, 3, s + 1)]
    if res == 32:  # lone voxels on a block face whose neighbouring block holds no voxel at all (~0 in cellBlocks): blocks (0,1,1), (1,0,1), (1,1,0) stay empty
        v += [(16, 20, 20), (20, 16, 20), (20, 20, 16)]
    else:  # blocks (2,2,2) and (3,3,3) stay empty; looked into from -X, -Y, -Z and from +X, +Y, +Z
        v += [(48, 40, 40), (40, 48, 40), (40, 40, 48), (47, 55, 55), (55, 47, 55), (55, 55, 47)]
    return np.array(v)


@pytest.mark.parametrize("res", [32, 64])
def test_cell_block_seams(mv, res):
    xyz = seam_set(res)
    blocks = {tuple(b) for b in xyz // 16}
    assert ((0, 1, 1) not in blocks and (1, 1, 0) not in blocks) if res == 32 else ((2, 2, 2) not in blocks and (3, 3, 3) not in blocks)
    svo, want = check(mv, xyz, res)
    assert svo.device_view().cellBlocks != 0  # the cell-index path ran
    m = dict(zip(map(tuple, want["xyz"]), want["masks"]))
    assert m[(15, 3, 3)] == 63 & ~(1 << 3) and m[(16, 3, 3)] == 63 & ~(1 << 5) and m[(3, 3, 15)] == 63 & ~(1 << 4)


# ---- launch seams: two voxels per thread, 64 lanes per wave, 256 voxels per group of the emit kernel, the blocks of the library scan -----------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 4097, 32769])
def test_voxel_counts(mv, n):
    """the first n cells of a 64^3 grid in Morton order: whole octants, so from 512 on there are interior voxels without faces"""
    check(mv, S.decode(np.arange(n, dtype=np.uint64)), 64)


def test_run_without_faces_across_a_group_boundary(mv):
    """a full 16^3 cube behind 40 loose voxels: the 4^3 block at (20..23)^3 is 64 consecutive voxels with mask 0 at vIndex 488..551, across a wave and a
    256-voxel group, so that offsets repeat over the boundary"""
    loose = [(2 * i % 14, 2 * (i // 7), 0) for i in range(40)]
    xyz = np.concatenate([np.array(loose), full(16) + 16])
    assert len({tuple(p) for p in loose}) == 40
    _, want = check(mv, xyz, 32)
    assert np.array_equal(want["xyz"][488], (20, 20, 20)) and np.array_equal(want["xyz"][551], (23, 23, 23)) and not want["masks"][488:552].any()


# ---- octrees without a cell index: neighbours by binary search ------------------------------------------------------------------------------------------------
def sparse_set(res, seed, n=3000):
    rng = np.random.default_rng(seed)
    xyz = rng.integers(0, res, size=(n, 3))
    near = xyz[:600].copy()  # adjacent pairs along every axis
    near[np.arange(600), np.arange(600) % 3] += np.where(near[np.arange(600), np.arange(600) % 3] < res - 1, 1, -1)
    e = res - 1
    edge = [(0, 0, 0), (e, e, e), (e, 0, 0), (e - 1, 0, 0), (0, e, 0), (0, e - 1, 0), (0, 0, e), (0, 0, e - 1), (e, e, 0), (0, e, e), (e, 0, e), (5, e, 7), (5, e, 8), (1, 0, 0)]
    return np.concatenate([xyz, near, edge])


@pytest.mark.parametrize("res", [1 << 15, 1 << 21])
def test_search_path_of_deep_octrees(mv, res):
    svo, want = check(mv, sparse_set(res, res % 1000), res)
    assert svo.info().levels > 14
    m = dict(zip(map(tuple, want["xyz"]), want["masks"]))
    assert m[(0, 0, 0)] == 63 & ~(1 << 3) and m[(res - 1,) * 3] == 63  # (1,0,0) is set; no wrap from gridRes - 1 to 0


CHILD = """
import sys
import numpy as np
sys.path.insert(0, %r)
import massivevoxelraytracing_amd as mv
xyz = np.load(sys.argv[1])
svo = mv.IntersectorOctreeGPU()
svo.build_voxels(xyz, None, gridRes=64)
masks, n = svo.surface_masks()
np.save(sys.argv[2], masks)
print("cellBlocks", svo.device_view().cellBlocks != 0, "faces", n)
"""


def test_same_masks_with_and_without_cell_index(mv, tmp_path):
    """MVRT_CELL_INDEX=0 in a child process (the knob is read by experiment builds of the library, tools/build_variant.sh; the product build ignores it and
    the child then repeats the default path) and, in this process, the tree flavour, which never has a cell index: the same gridRes-64 set, the same masks"""
    rng = np.random.default_rng(5)
    xyz = np.concatenate([np.argwhere(rng.random((64, 64, 64)) < 0.03), seam_set(64)]).astype(np.uint32)
    svo, want = check(mv, xyz, 64)
    assert svo.device_view().cellBlocks != 0
    tree = build(mv, xyz, 64, flags=3)
    assert tree.info().flavour == 2
    assert_surface(tree, want)
    np.save(tmp_path / "xyz.npy", xyz)
    out = subprocess.check_output([sys.executable, "-c", CHILD % ROOT, str(tmp_path / "xyz.npy"), str(tmp_path / "masks.npy")], env=dict(os.environ, MVRT_CELL_INDEX="0"),
                                  timeout=120).decode()
    print(out.strip())
    # the child says which path it took: in a product build the one with the cell index again, so there only the tree flavour above compares the two paths
    assert out.strip().splitlines()[-1].split() in (["cellBlocks", "True", "faces", str(want["nFaces"])], ["cellBlocks", "False", "faces", str(want["nFaces"])])
    assert np.array_equal(np.load(tmp_path / "masks.npy"), want["masks"])


# ---- flavours: the bunny at 64^3 from triangles ---------------------------------------------------------------------------------------------------------------
def test_flavours_of_a_triangle_build(mv):
    """The model's input is the library's own read_voxels output (checked against the oracle in test_gpu_build.py), so this compares the surface calls with
    the model on the set the build made; the + / - face balance below holds for any voxel set and needs neither."""
    tris = bunny_tris()
    v = tris.reshape(-1, 3)
    lo = v.min(0)
    dps = np.float32((v.max(0) - lo).max() / np.float32(64))
    B = mv.IntersectorOctreeGPU
    same_set = (B.BUILD_NO_DAG, B.BUILD_NO_EMBEDDED_MASK, B.BUILD_NO_DAG | B.BUILD_NO_EMBEDDED_MASK)
    got = {}
    for flags in (0,) + same_set + (B.BUILD_CONSERVATIVE,):
        svo = mv.IntersectorOctreeGPU()
        svo.build(v, None, None, None, lo, dps, 64, flags=flags)
        xyz, _ = svo.read_voxels()
        want = S.surface(xyz, 64, lo, dps)
        assert np.array_equal(want["xyz"], xyz)  # read_voxels is in vIndex order
        assert_surface(svo, want)
        got[flags] = want
        count = np.bincount(want["faceDir"], minlength=6)
        assert count[3] == count[5] and count[1] == count[0] and count[4] == count[2]  # per axis as many + faces as - faces, whatever the model says
    assert all(np.array_equal(got[f]["masks"], got[0]["masks"]) for f in same_set)  # the masks depend on the voxel set only
    # the conservative voxelization is another set, a proper superset; a thicker shell has more voxels but need not have more faces (here it has fewer)
    six, cons = got[0], got[B.BUILD_CONSERVATIVE]
    assert len(cons["xyz"]) > len(six["xyz"]) and np.isin(S.morton(six["xyz"]), S.morton(cons["xyz"])).all()


# ---- edits ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_after_edits(mv):
    rng = np.random.default_rng(8)
    old = np.concatenate([np.argwhere(rng.random((64, 64, 64)) < 0.02), seam_set(64)])
    svo, _ = check(mv, old, 64)
    # structural: remove one voxel of each seam pair and a tenth of the rest, insert neighbours across the seams x = 15|16 and z = 31|32
    gone = np.concatenate([np.array([(16, 3, 3), (3, 15, 3), (3, 3, 32)]), old[rng.random(len(old)) < 0.1]])
    fresh = np.array([(15, 9, 9), (16, 9, 9), (15, 3, 4), (9, 9, 31), (9, 9, 32), (47, 40, 40)])
    svo.edit_voxels(np.concatenate([gone, fresh]).astype(np.uint32), None, np.concatenate([np.zeros(len(gone), np.uint8), np.ones(len(fresh), np.uint8)]))
    keep = {tuple(p) for p in old} - {tuple(p) for p in gone} | {tuple(p) for p in fresh}
    want = S.surface(np.array(sorted(keep)), 64, LOWER, DPS)
    assert svo.info().numberOfVoxels == len(want["xyz"])
    assert_surface(svo, want)
    # attribute-only: the geometry is unchanged
    attrs = rng.integers(0, 256, size=(50, 8), dtype=np.uint8)
    svo.edit_voxels(want["xyz"][:50].astype(np.uint32), attrs)
    assert np.array_equal(svo.read_voxels()[1][:50, :3], attrs[:, :3])
    assert_surface(svo, want)


# ---- the contract of the calls ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(mv):
    rng = np.random.default_rng(12)
    xyz = np.argwhere(rng.random((16, 16, 16)) < 0.3)
    return build(mv, xyz, 16), S.surface(xyz, 16, LOWER, DPS)


def test_capacity_one_short(mv, small):
    svo, want = small
    n, m = want["nFaces"], len(want["vertices"])
    outs = {k: filled(mv, s, t) for k, s, t in (("fv", n, np.uint32), ("fd", n, np.uint8), ("pos", (n, 12), np.float32), ("idx", (n, 4), np.uint32), ("vtx", (m, 3), np.float32))}
    nf, nv = C.c_uint64(0), C.c_uint64(0)
    lib = mv.lib()
    assert lib.mvrt_svo_surface_quads(svo._h, n - 1, outs["fv"][0].ptr, outs["fd"][0].ptr, outs["pos"][0].ptr, C.byref(nf), None) != 0
    assert nf.value == n and b"faceCapacity %d" % (n - 1) in lib.mvrt_last_error() and b"%d faces" % n in lib.mvrt_last_error()
    for caps, what in (((n - 1, m), b"faceCapacity"), ((n, m - 1), b"vertexCapacity")):
        nf.value = nv.value = 0
        assert lib.mvrt_svo_surface_mesh(svo._h, caps[0], caps[1], outs["fv"][0].ptr, outs["fd"][0].ptr, outs["idx"][0].ptr, outs["vtx"][0].ptr, C.byref(nf), C.byref(nv), None) != 0
        assert (nf.value, nv.value) == (n, m) and what in lib.mvrt_last_error()
    for dev, host in outs.values():
        assert np.array_equal(dev.to_host().view(np.uint8), host.view(np.uint8))  # nothing was written
    with pytest.raises(mv.MvrtError, match="faceCapacity"):
        svo.surface_quads_device(n - 1, outs["fv"][0])
    # a larger capacity than the count is fine and writes the count's worth
    assert svo.surface_quads_device(n + 7, mv.DeviceArray(n + 7, np.uint32)) == n


def test_null_outputs(mv, small):
    svo, want = small
    n, m = want["nFaces"], len(want["vertices"])
    assert svo.surface_quads_device() == n and svo.surface_mesh_device() == (n, m)  # sizing calls: capacity 0, all NULL
    fd = mv.DeviceArray(n, np.uint8)
    assert svo.surface_quads_device(n, None, fd, None) == n and np.array_equal(fd.to_host(), want["faceDir"])
    pos = mv.DeviceArray((n, 4, 3), np.float32)
    svo.surface_quads_device(n, None, None, pos)
    assert np.array_equal(bits(pos.to_host()), bits(want["positions"]))
    idx = mv.DeviceArray((n, 4), np.uint32)
    assert svo.surface_mesh_device(n, 0, None, None, idx, None) == (n, m) and np.array_equal(idx.to_host(), want["indices"])  # no vertices: their capacity is not looked at
    vtx, fv = mv.DeviceArray((m, 3), np.float32), mv.DeviceArray(n, np.uint32)
    svo.surface_mesh_device(0, m, None, None, None, vtx)
    assert np.array_equal(bits(vtx.to_host()), bits(want["vertices"]))
    svo.surface_mesh_device(n, 0, fv, None, None, None)
    assert np.array_equal(fv.to_host(), want["faceVoxel"])
    assert mv.lib().mvrt_svo_surface_masks(svo._h, None, None, None) == 0  # even the count may be NULL


def test_positions_at_an_odd_address(mv, small):
    """a positions array that is not 16-byte aligned takes the scalar stores"""
    svo, want = small
    n = want["nFaces"]
    buf = mv.DeviceArray(n * 12 + 1, np.float32)
    svo.surface_quads_device(n, None, None, buf.ptr + 4)
    assert np.array_equal(bits(buf.to_host()[1:]), bits(want["positions"]).reshape(-1))


def test_refusals_without_gpu_work(mv, small):
    svo, _ = small
    empty = mv.IntersectorOctreeGPU()
    nodes, attrs, _ = svo.download()
    i = svo.info()
    up = mv.IntersectorOctreeGPU()
    up.upload(nodes, attrs, LOWER, DPS, 16, i.hasEmission, embeddedMask=bool(i.embeddedMask))
    before = mv.allocation_state()[2]
    for h, text in ((empty, "no octree"), (up, "keeps no Morton codes")):
        for call in (h.surface_masks_device, h.surface_quads_device, h.surface_mesh_device):
            with pytest.raises(mv.MvrtError, match=text):
                call()
    assert mv.allocation_state()[2] == before
    with pytest.raises(mv.MvrtError, match="keeps no Morton codes"):
        up.read_voxels()  # the same reason as read_voxels


def test_the_handle_is_not_modified(mv, small):
    svo, want = small
    before = svo.download(want_morton=True)
    held = mv.allocation_state()[:2]
    assert_surface(svo, want)
    assert all(np.array_equal(a, b) for a, b in zip(svo.download(want_morton=True), before))
    assert mv.allocation_state()[:2] == held  # the scratch is gone


# ---- upper layers ---------------------------------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_runs(tmp_path, mv):
    exe, libdir = common.compile_usage(tmp_path, "surface_usage")
    out = subprocess.check_output([str(exe), "run"], timeout=120).decode()
    assert "voxels 8 masks 8 first 37 faces 24 counted 24 quads 24 vertices 26 indices 96 same 1" in out


@pytest.mark.parametrize("weld", [True, False])
def test_voxel_mesh_app(tmp_path, mv, weld):
    from massivevoxelraytracing_amd import build as b
    b.build_apps(verbose=False)
    tris = bunny_tris()
    v = tris.reshape(-1, 3)
    with open(tmp_path / "bunny.obj", "w") as f:
        f.write("".join("v %.9g %.9g %.9g\n" % tuple(p) for p in v) + "".join("f %d %d %d\n" % (3 * t + 1, 3 * t + 2, 3 * t + 3) for t in range(len(tris))))
    out = subprocess.check_output([os.path.join(ROOT, "apps", "voxel_mesh"), str(tmp_path / "bunny.obj"), "64", str(tmp_path / "bunny.ply")] + ([] if weld else ["--no-weld"]),
                                  timeout=120).decode()
    lo = v.min(0)
    svo = mv.IntersectorOctreeGPU()
    svo.build(v, None, None, None, lo, np.float32((v.max(0) - lo).max() / np.float32(64)), 64)
    vertices, indices, colours = S.read_ply_quads(tmp_path / "bunny.ply")
    _, attrs = svo.read_voxels()
    if weld:
        m = svo.surface_mesh()
        assert np.array_equal(bits(vertices), bits(m["vertices"])) and np.array_equal(indices, m["indices"])
    else:
        m = svo.surface_quads()
        assert np.array_equal(bits(vertices), bits(m["positions"].reshape(-1, 3))) and np.array_equal(indices.reshape(-1), np.arange(len(indices) * 4))
    assert np.array_equal(colours, attrs[m["faceVoxel"], :3])
    assert "faces %d vertices %d" % (len(indices), len(vertices)) in out
