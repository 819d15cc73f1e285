"""Exterior masks and caller-supplied face masks on the GPU (mvrt_svo_surface_exterior_masks, mvrt_svo_surface_quads_masked / _mesh_masked / _merged_masked)
against the numpy models of tests/exterior_expected.py, surface_expected.py and merge_expected.py, bit for bit, on the smallest inputs that can break each
mechanism: grids without a gap, single voxels and odd counts, the cage and its open variants, diagonal contact, a shell on the grid border, nested shells, one
long gap, several hundred chained gaps, random fills, voxel counts around the 256-voxel launch blocks with a cage among the last voxels, the 21-bit edge, every
flavour, edits, a rebuilt upload, the bunny -- and the contract of the calls (counts only, capacities, refusals, a handle that is never modified)."""
import ctypes as C
import functools

import numpy as np
import pytest

import exterior_expected as E
import fill_expected as F
import merge_expected as M
import surface_expected as S
from common import bunny_tris
from fixtures import mv  # noqa: F401 (fixtures)
from voxel_sets import CAGE, DPS, LOWER, filled, filler, full, serpentine, shell, tube

pytestmark = pytest.mark.gpu

ALL_FLAGS = (0, M.ANY_ATTRIBUTE, M.WELD, M.ANY_ATTRIBUTE | M.WELD)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def build(mv, xyz, res, flags=0, attribs=None):
    svo = mv.IntersectorOctreeGPU()
    svo.build_voxels(np.ascontiguousarray(xyz, np.uint32), attribs, origin=LOWER, dps=DPS, gridRes=res, flags=flags)
    return svo


def assert_exterior(svo, want):
    """masks, nFaces, nHidden and the counts-only call == the model"""
    masks, nf, nh = svo.surface_exterior_masks()
    print("voxels", len(masks), "faces", nf, "hidden", nh, "model", want["nFaces"], want["nHidden"])
    assert masks.dtype == np.uint8 and masks.shape == want["masks"].shape and np.array_equal(masks, want["masks"])
    assert (nf, nh) == (want["nFaces"], want["nHidden"])
    assert svo.surface_exterior_masks_device() == (want["nFaces"], want["nHidden"])  # masksDev NULL
    return masks


def check(mv, xyz, res, flags=0):
    want = E.exterior(xyz, res)
    svo = build(mv, xyz, res, flags)
    assert_exterior(svo, want)
    return svo, want


# ---- tiny grids, single voxels, odd counts, the cage, diagonal contact, the border ------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [2, 4])
def test_grids_without_a_gap(mv, res):
    _, want = check(mv, full(res), res)
    assert want["nHidden"] == 0 and want["nFaces"] == 6 * res * res
    _, want = check(mv, [(1, 0, 1)], res)  # n = 1
    assert want["masks"].tolist() == [0x3F]
    _, want = check(mv, [(0, 0, 0), (res - 1, 0, 0), (0, res - 1, res - 1)], res)  # odd n: the last thread of the masks kernel holds one voxel
    assert want["nFaces"] == (18 if res > 2 else 16) and want["nHidden"] == 0


def test_cage_and_its_open_variants(mv):
    _, want = check(mv, CAGE, 4)
    assert (want["nFaces"], want["nHidden"]) == (30, 6) and (want["masks"] != 0).all()
    for gone in range(6):
        _, w = check(mv, CAGE[:gone] + CAGE[gone + 1:], 4)
        assert (w["nFaces"], w["nHidden"]) == (30, 0) and np.array_equal(w["masks"], w["plain"])


def test_diagonal_contact(mv):
    solid = np.ones((4, 4, 3), bool)
    solid[1, 1, 1] = solid[2, 2, 1] = False
    _, want = check(mv, np.argwhere(solid), 8)
    assert (want["nFaces"], want["nHidden"]) == (80, 12) and (want["masks"] == 0).sum() == 2


def test_shell_on_the_grid_border(mv):
    _, want = check(mv, shell(0, 8), 8)
    assert (want["nFaces"], want["nHidden"]) == (384, 216)


def test_nested_shells_the_inner_one_has_no_exterior_face(mv):
    _, want = check(mv, np.concatenate([shell(2, 14), shell(5, 11)]), 16)
    assert (want["nFaces"], want["nHidden"]) == (864, 912) and (want["masks"] == 0).sum() == 152


def test_one_long_gap_and_the_same_opened(mv):
    t = tube()
    _, want = check(mv, t, 512)
    assert (want["nFaces"], want["nHidden"]) == (3618, 1194)
    cap = (t == (399, 11, 21)).all(1)
    svo, w = check(mv, t[~cap], 512)
    assert w["nHidden"] == 0 and np.array_equal(svo.surface_exterior_masks()[0], svo.surface_masks()[0])  # identical to the plain masks


def test_many_chained_gaps_sealed_and_opened(mv):
    solid, path = serpentine()
    _, want = check(mv, np.argwhere(solid), 32)
    assert want["nFaces"] == 6 * 32 * 32 and want["nHidden"] > 2 * len(path)  # only the outside of the block
    end = path[-1].copy()
    end[0] = 0 if end[0] == 1 else 31
    opened = solid.copy()
    opened[tuple(end)] = False
    _, w = check(mv, np.argwhere(opened), 32)
    assert w["nHidden"] == 0


# ---- random fills ----------------------------------------------------------------------------------------------------------------------------------------------------
def random_set(res, density, seed):
    rng = np.random.default_rng(1000 * res + 10 * int(density * 10) + seed)
    xyz = np.argwhere(rng.random((res, res, res)) < density)
    border = [(0, 1, 2), (res - 1, 2, 1), (1, 0, 2), (2, res - 1, 1), (2, 1, 0), (1, 2, res - 1)]
    return np.concatenate([xyz, border])


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("density", [0.5, 0.7, 0.85])
@pytest.mark.parametrize("res", [16, 32])
def test_random_fill(mv, res, density, seed):
    _, want = check(mv, random_set(res, density, seed), res)
    assert want["nHidden"] >= 164


# ---- the launch blocks -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_voxel_counts_at_the_block_seams(mv, n):
    """n voxels at gridRes 32 whose last six in Morton order are a cage in the top octant: its voxels lie on both sides of the 256-voxel seam where n says so"""
    cage = np.array(CAGE) + 28
    xyz = np.concatenate([filler(n - 6, 4), cage])
    assert len(np.unique(xyz, axis=0)) == n
    svo, want = check(mv, xyz, 32)
    assert np.array_equal(want["xyz"][-6:], S.sorted_voxels(cage)) and want["nHidden"] == 6
    assert (want["masks"][-6:] != want["plain"][-6:]).all() and np.array_equal(want["masks"][:-6], want["plain"][:-6])


# ---- the 21-bit edge -------------------------------------------------------------------------------------------------------------------------------------------------
def test_far_corner_of_the_largest_grid(mv):
    res = 1 << 21
    svo, want = check(mv, shell(res - 5, res), res)  # 63-bit keys; the + neighbours of the outer faces lie outside the grid
    assert svo.info().levels == 21 and (want["nFaces"], want["nHidden"]) == (150, 54)


# ---- flavours, edits, uploads, triangle builds -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed():
    rng = np.random.default_rng(77)
    xyz = np.concatenate([np.argwhere(rng.random((32, 32, 32)) < 0.7), shell(3, 12)])
    return xyz, E.exterior(xyz, 32)


@pytest.mark.parametrize("flags", [1, 2, 3])
def test_every_flavour_gives_the_same_bytes(mv, mixed, flags):
    xyz, want = mixed
    assert want["nHidden"] > 1000
    svo = build(mv, xyz, 32, flags)
    assert flags != 3 or svo.info().flavour == 2  # the tree flavour
    assert np.array_equal(assert_exterior(svo, want), assert_exterior(build(mv, xyz, 32, 0), want))


def test_after_edits_seal_and_unseal_a_cavity(mv):
    at = np.array(CAGE) + 3
    svo, want = check(mv, at[:5], 8)
    assert want["nHidden"] == 0
    svo.edit_voxels(at[5:].astype(np.uint32))
    sealed = E.exterior(at, 8)
    assert sealed["nHidden"] == 6
    assert_exterior(svo, sealed)
    svo.edit_voxels(at[2:3].astype(np.uint32), None, np.zeros(1, np.uint8))
    assert_exterior(svo, E.exterior(np.delete(at, 2, axis=0), 8))


def test_upload_and_empty_handle_are_refused_and_a_rebuilt_upload_works(mv, mixed):
    xyz, want = mixed
    svo = build(mv, xyz, 32)
    nodes, attrs, _ = svo.download()
    i = svo.info()
    up = mv.IntersectorOctreeGPU()
    up.upload(nodes, attrs, LOWER, DPS, 32, i.hasEmission, embeddedMask=bool(i.embeddedMask))
    masks = mv.DeviceArray.from_host(want["masks"])
    before = mv.allocation_state()[2]
    for h, text in ((mv.IntersectorOctreeGPU(), "no octree"), (up, "keeps no Morton codes")):
        for call in (h.surface_exterior_masks_device, lambda: h.surface_quads_device(masks=masks), lambda: h.surface_mesh_device(masks=masks),
                     lambda: h.surface_merged_device(masks=masks)):
            with pytest.raises(mv.MvrtError, match=text):
                call()
    with pytest.raises(mv.MvrtError, match="null masksDev"):
        mv._check(mv.lib().mvrt_svo_surface_quads_masked(svo._h, None, 0, None, None, None, None, None))
    assert mv.allocation_state()[2] == before  # refused before any GPU work
    up.rebuild()
    assert_exterior(up, want)


def test_the_handle_is_not_modified(mv, mixed):
    xyz, want = mixed
    svo = build(mv, xyz, 32)
    before = svo.download(want_morton=True)
    info = bytes(svo.info())
    held = mv.allocation_state()[:2]
    masks = assert_exterior(svo, want)
    svo.surface_quads(masks=masks), svo.surface_mesh(masks=masks), svo.surface_merged(M.WELD, masks=masks)
    assert bytes(svo.info()) == info and all(np.array_equal(a, b) for a, b in zip(svo.download(want_morton=True), before))
    assert mv.allocation_state()[:2] == held  # the scratch is gone


@pytest.mark.parametrize("conservative", [False, True])
def test_bunny_from_triangles(mv, conservative):
    tris = bunny_tris()
    v = tris.reshape(-1, 3)
    lo = v.min(0)
    dps = np.float32((v.max(0) - lo).max() / np.float32(64))
    svo = mv.IntersectorOctreeGPU()
    svo.build(v, None, None, None, lo, dps, 64, flags=mv.IntersectorOctreeGPU.BUILD_CONSERVATIVE if conservative else 0)
    xyz, _ = svo.read_voxels()
    want = E.exterior(xyz, 64)
    assert_exterior(svo, want)
    if not conservative:
        assert (len(xyz), want["nFaces"] + want["nHidden"], want["nFaces"]) == (8516, 27550, 14558)  # the oracle's numbers (tests/test_exterior_cpu.py)


# ---- the _masked calls with exterior masks, against the models ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene(name):
    """-> (xyz, res, attrs (n, 8) uint8 in the given order)"""
    if name == "nested":
        xyz, res = np.concatenate([shell(2, 14), shell(5, 11)]), 16
    elif name == "random":
        xyz, res = random_set(16, 0.7, 1), 16
    else:
        xyz, res = np.concatenate([np.array(CAGE), np.array(CAGE) + (3, 0, 0), [(7, 7, 7)]]), 8
    rng = np.random.default_rng(len(xyz))
    attrs = np.array([(200, 10, 10, 255, 0, 0, 0, 255), (10, 10, 200, 255, 0, 0, 0, 255)], np.uint8)[rng.integers(0, 2, size=len(xyz))]
    return xyz, res, attrs


@pytest.mark.parametrize("name", ["cages", "nested", "random"])
def test_masked_calls_with_exterior_masks_against_the_models(mv, name):
    xyz, res, attrs = scene(name)
    svo = build(mv, xyz, res, 0, attrs)
    want = E.exterior(xyz, res)
    ext = mv.DeviceArray.from_host(assert_exterior(svo, want))
    v = want["xyz"]
    fv, fd, corners = S.faces(v, want["masks"])
    assert len(fv) == want["nFaces"] > 0 and want["nHidden"] > 0
    q = svo.surface_quads(masks=ext)
    assert svo.surface_quads_device(masks=ext) == len(fv)  # the sizing call: the popcount of the given masks
    assert np.array_equal(q["faceVoxel"], fv) and np.array_equal(q["faceDir"], fd) and np.array_equal(bits(q["positions"]), bits(S.positions(corners, LOWER, DPS)))
    vertices, indices = S.weld(corners, res, LOWER, DPS)
    m = svo.surface_mesh(masks=ext)
    assert svo.surface_mesh_device(masks=ext) == (len(fv), len(vertices))
    assert np.array_equal(m["faceVoxel"], fv) and np.array_equal(m["faceDir"], fd) and np.array_equal(m["indices"], indices) and np.array_equal(bits(m["vertices"]), bits(vertices))
    # merged: the model on the filled set (E2), its rectVoxel mapped back through coordinates: the rectangles depend only on the faces and their voxels' attributes
    _, own_attrs = svo.read_voxels()
    f = S.sorted_voxels(F.filled_set(v, res))
    own = np.isin(S.morton(f), S.morton(v))
    f_attrs = np.zeros((len(f), 8), np.uint8)
    f_attrs[own] = own_attrs
    back = np.cumsum(own) - 1  # index in the filled set -> vIndex, for the voxels that were there before
    for flags in ALL_FLAGS:
        w = M.merged(f, f_attrs, res, LOWER, DPS, flags)
        assert own[w["rectVoxel"]].all()  # a filled cell owns no face
        got = svo.surface_merged(flags, masks=ext)
        n = len(w["rectVoxel"])
        assert svo.surface_merged_device(flags, masks=ext) == (len(fv), n, len(w["vertices"]) if flags & M.WELD else 0)
        assert got["nFaces"] == len(fv) and np.array_equal(got["rectVoxel"], back[w["rectVoxel"]]) and np.array_equal(got["rectDir"], w["rectDir"]), flags
        assert np.array_equal(got["rectSize"], w["rectSize"]) and np.array_equal(bits(got["positions"]), bits(w["positions"])), flags
        if flags & M.WELD:
            assert np.array_equal(got["indices"], w["indices"]) and np.array_equal(bits(got["vertices"]), bits(w["vertices"])), flags


@pytest.mark.parametrize("name", ["cages", "random"])
def test_masked_calls_with_plain_masks_equal_the_unmasked_calls(mv, name):
    xyz, res, attrs = scene(name)
    svo = build(mv, xyz, res, 0, attrs)
    plain, n = svo.surface_masks()
    for kw in (dict(masks=plain), dict(masks=mv.DeviceArray.from_host(plain))):  # a numpy array and a device array
        pairs = [(svo.surface_quads(), svo.surface_quads(**kw)), (svo.surface_mesh(), svo.surface_mesh(**kw))]
        pairs += [(svo.surface_merged(flags), svo.surface_merged(flags, **kw)) for flags in ALL_FLAGS]
        for a, b in pairs:
            assert a.keys() == b.keys()
            for k in a:  # byte for byte
                assert (a[k].tobytes() == b[k].tobytes() and a[k].shape == b[k].shape) if isinstance(a[k], np.ndarray) else a[k] == b[k], k
    assert svo.surface_quads_device(masks=plain) == n


# ---- arbitrary masks ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_masks_are_taken_as_given(mv):
    svo = build(mv, full(2), 2)
    xyz = S.sorted_voxels(full(2))
    every = np.full(8, 0x3F, np.uint8)
    q = svo.surface_quads(masks=every)  # a bit whose neighbour is occupied still yields its face
    fv, fd, corners = S.faces(xyz, every)
    assert len(fv) == 48 and np.array_equal(q["faceVoxel"], fv) and np.array_equal(q["faceDir"], fd) and np.array_equal(bits(q["positions"]), bits(S.positions(corners, LOWER, DPS)))
    high = svo.surface_quads(masks=np.full(8, 0xFF, np.uint8))  # bits 6 and 7 are ignored
    assert all(np.array_equal(q[k], high[k]) for k in q) and svo.surface_quads_device(masks=np.full(8, 0xC0, np.uint8)) == 0
    up = svo.surface_quads(masks=np.full(8, 0x02, np.uint8))  # one direction only
    assert up["faceDir"].tolist() == [1] * 8 and up["faceVoxel"].tolist() == list(range(8))
    mesh = svo.surface_mesh(masks=np.full(8, 0x02, np.uint8))
    assert len(mesh["vertices"]) == 18 and mesh["indices"].shape == (8, 4)  # two layers of 3 x 3 corners
    merged = svo.surface_merged(M.WELD, masks=np.full(8, 0x02, np.uint8))
    assert merged["nFaces"] == 8 and merged["rectSize"].tolist() == [[2, 2], [2, 2]] and len(merged["vertices"]) == 8


def test_all_zero_masks_succeed_and_write_nothing(mv):
    svo = build(mv, full(2), 2)
    zero = mv.DeviceArray.from_host(np.zeros(8, np.uint8))
    (fv, fv_host), (fd, fd_host), (pos, pos_host) = filled(mv, 4, np.uint32), filled(mv, 4, np.uint8), filled(mv, (4, 4, 3), np.float32)
    assert svo.surface_quads_device(4, fv, fd, pos, masks=zero) == 0
    assert svo.surface_mesh_device(4, 4, fv, fd, fv, pos, masks=zero) == (0, 0)
    assert svo.surface_merged_device(M.WELD, 4, 4, fv, fd, None, pos, fv, None, masks=zero) == (0, 0, 0)
    assert np.array_equal(fv.to_host(), fv_host) and np.array_equal(fd.to_host(), fd_host) and np.array_equal(bits(pos.to_host()), bits(pos_host))


def test_capacity_one_short(mv, mixed):
    xyz, want = mixed
    svo = build(mv, xyz, 32)
    ext = mv.DeviceArray.from_host(want["masks"])
    n = want["nFaces"]
    (fv, fv_host), (fd, fd_host), (pos, pos_host) = filled(mv, n, np.uint32), filled(mv, n, np.uint8), filled(mv, (n, 4, 3), np.float32)
    lib = mv.lib()
    nf = C.c_uint64(0)
    assert lib.mvrt_svo_surface_quads_masked(svo._h, ext.ptr, n - 1, fv.ptr, fd.ptr, pos.ptr, C.byref(nf), None) != 0
    err = lib.mvrt_last_error()
    assert nf.value == n and b"mvrt_svo_surface_quads_masked: faceCapacity %d" % (n - 1) in err and b"%d faces" % n in err
    assert np.array_equal(fv.to_host(), fv_host) and np.array_equal(fd.to_host(), fd_host) and np.array_equal(bits(pos.to_host()), bits(pos_host))  # nothing was written
    with pytest.raises(mv.MvrtError, match="mvrt_svo_surface_mesh_masked: faceCapacity"):
        svo.surface_mesh_device(n - 1, 8 * n, fv, fd, None, None, masks=ext)
    with pytest.raises(mv.MvrtError, match="mvrt_svo_surface_merged_masked: rectCapacity 1 "):
        svo.surface_merged_device(0, 1, 0, fv, fd, None, None, masks=ext)
    assert np.array_equal(fv.to_host(), fv_host) and np.array_equal(fd.to_host(), fd_host)
    assert svo.surface_quads_device(n, fv, fd, pos, masks=ext) == n  # and with room for all of them
    assert np.array_equal(fv.to_host(), S.faces(want["xyz"], want["masks"])[0])


def test_ao_of_the_exterior_faces_is_the_plain_bake_of_the_kept_faces(mv):
    xyz = np.concatenate([shell(8, 24), [(2, 3, 4), (29, 30, 28)]])
    svo = build(mv, xyz, 32)
    want = E.exterior(xyz, 32)
    plain = svo.surface_ao(samples=16)
    got = svo.surface_ao(samples=16, masks=want["masks"])
    pv, pd, _ = S.faces(want["xyz"], want["plain"])
    assert np.array_equal(plain["faceVoxel"], pv) and np.array_equal(plain["faceDir"], pd)
    kept = ((want["masks"][pv] >> pd) & 1).astype(bool)
    assert kept.sum() == want["nFaces"] < len(pv)
    assert np.array_equal(got["faceVoxel"], pv[kept]) and np.array_equal(got["faceDir"], pd[kept]) and np.array_equal(got["open"], plain["open"][kept])
