"""mvrt_svo_surface_smooth on the GPU against the numpy model of tests/smooth_expected.py: faceVoxel, faceDir, indices, neighbours, displacements and the clamp
count as integers, the vertices by their bits, on the smallest inputs that can break each mechanism -- corners on both grid borders, non-manifold vertices of
degree 5 and 6, both parities of the two displacement buffers, several workgroups with a partial last one, every limit and both weight pairs, exterior and
random caller masks (open surfaces, degree 2, faces listed from both sides), the 2^21 grid, every flavour, and the contract of the call."""
import ctypes as C

import numpy as np
import pytest

import smooth_expected as M
import surface_expected as S
from common import bunny_tris
from fixtures import mv  # noqa: F401 (fixtures)
from voxel_sets import DPS, LOWER, block_and_noise, build, filled

pytestmark = pytest.mark.gpu

KEYS = ("faceVoxel", "faceDir", "indices", "neighbours", "displacements")
TAUBIN = (128, -136)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_smooth(got, want):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    assert np.array_equal(bits(got["vertices"]), bits(want["vertices"])) and got["clamped"] == want["clamped"]


def check(mv, xyz, res, K=4, weights=(256, 256), limit=127, masks=None, svo=None, lower=LOWER, dps=DPS):
    want = M.smooth(xyz, res, lower, dps, K, weights, limit, masks)
    svo = build(mv, xyz, res) if svo is None else svo
    assert svo.info().numberOfVoxels == len(want["xyz"])
    assert_smooth(svo.surface_smooth(K, weights, limit, masks=masks), want)
    return svo, want


def degrees(want):
    return sorted({bin(m).count("1") for m in want["neighbours"]})


# ---- tiny sets ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xyz", [[(0, 0, 0)], [(1, 1, 1)], [(0, 0, 0), (1, 1, 1)]])
@pytest.mark.parametrize("K", [1, 6])
def test_grid_of_two(mv, xyz, K):
    """the corners lie on both grid borders, coordinate gridRes included"""
    _, want = check(mv, xyz, 2, K)
    assert want["corners"].min() == (0 if (0, 0, 0) in xyz else 1) and want["corners"].max() == (2 if (1, 1, 1) in xyz else 1)


@pytest.mark.parametrize("xyz,res", [([(0, 0, 0)], 2), ([(0, 0, 0), (3, 3, 3), (3, 0, 2)], 4), ([(0, 0, 0), ((1 << 21) - 1,) * 3], 1 << 21)])
@pytest.mark.parametrize("weights,K", [((-256, -256), 4), ((-256, 128), 3)])
def test_negative_weights_on_border_voxels(mv, xyz, res, weights, K):
    """a negative even weight moves the corners of a border voxel out of the grid: q = 256 c + d is negative at coordinate 0 and beyond 256 gridRes at the far
    border, and the position is compared by its bits"""
    _, want = check(mv, xyz, res, K, weights)
    q = M.fixed_point(want)
    assert q.min() < 0 and q.max() > 256 * want["corners"].max() - 1 and (weights != (-256, -256) or q.min() == -127)
    if res > 2:
        assert q.max() > 256 * res


def test_non_manifold_vertices(mv):
    _, edge = check(mv, [(1, 1, 1), (2, 2, 1)], 4, 5)  # two voxels that share an edge only
    assert degrees(edge) == [3, 5] and len(edge["corners"]) == 14
    _, corner = check(mv, [(1, 1, 1), (2, 2, 2)], 4, 5)  # ... a corner only
    assert degrees(corner) == [3, 6] and len(corner["corners"]) == 15


# ---- balls ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ball16(mv):
    return build(mv, M.ball(16, 6.3), 16)


@pytest.fixture(scope="module")
def ball32(mv):
    return build(mv, M.ball(32, 13.7), 32)


@pytest.mark.parametrize("K", [0, 1, 2, 3, 4])
def test_both_parities_of_the_buffers(mv, ball16, K):
    _, want = check(mv, M.ball(16, 6.3), 16, K, svo=ball16)
    assert len(want["corners"]) == 722 and (want["clamped"] == 192 if K == 4 else True)


@pytest.mark.parametrize("limit", [0, 64, 127, 128])
@pytest.mark.parametrize("weights,K", [((256, 256), 4), (TAUBIN, 7)])
def test_several_workgroups_weights_and_limits(mv, ball32, weights, K, limit):
    _, want = check(mv, M.ball(32, 13.7), 32, K, weights, limit, svo=ball32)
    assert len(want["corners"]) == 3554 and len(want["corners"]) % 256 != 0
    if limit == 0:
        assert not want["displacements"].any()


def test_no_iteration_is_the_plain_mesh(mv, ball32):
    got, plain = ball32.surface_smooth(0), ball32.surface_mesh()
    assert np.array_equal(bits(got["vertices"]), bits(plain["vertices"])) and got["clamped"] == 0 and not got["displacements"].any()
    for k in ("indices", "faceVoxel", "faceDir"):
        assert np.array_equal(got[k], plain[k])


# ---- masks ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_hollow_ball_plain_and_exterior(mv):
    g = M.ball(24, 10.2)
    inner = {tuple(p) for p in M.ball(24, 7.2).tolist()}
    xyz = np.array([p for p in g.tolist() if tuple(p) not in inner])
    svo, both = check(mv, xyz, 32)  # (the cells of [0, 24)^3 in the grid of 32) both surfaces smooth independently
    ext, nf, hidden = svo.surface_exterior_masks()
    assert hidden > 0 and nf + hidden == len(both["faceVoxel"])
    _, outer = check(mv, xyz, 32, masks=ext, svo=svo)
    assert len(outer["faceVoxel"]) == nf and len(outer["corners"]) < len(both["corners"])  # the inner surface is gone
    solid = M.smooth(g, 32, LOWER, DPS)
    assert np.array_equal(outer["corners"], solid["corners"]) and np.array_equal(outer["displacements"], solid["displacements"])  # ... and the outer one is the full ball's


@pytest.mark.parametrize("seed", [0, 1])
def test_random_caller_masks(mv, seed):
    """open surfaces, vertices of degree 2, faces listed from both sides"""
    xyz, _ = block_and_noise(seed, 32)
    masks = np.random.default_rng(40 + seed).integers(0, 64, len(S.sorted_voxels(xyz)), dtype=np.uint8)
    _, want = check(mv, xyz, 32, 5, TAUBIN, 127, masks=masks)
    assert 2 in degrees(want) and 6 in degrees(want)


# ---- the largest grid -----------------------------------------------------------------------------------------------------------------------------------------
def test_grid_of_two_to_the_21(mv):
    """int32 headroom of 256 c + d, 64-bit corner keys, the float conversion of q up to 2^29 + 128"""
    R = 1 << 21
    e = R - 1
    xyz = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 1), (e, e, e), (e - 1, e, e), (e, e - 1, e), (e - 1, e - 1, e - 1)]
    for K, weights in ((3, (256, 256)), (4, TAUBIN)):
        _, want = check(mv, xyz, R, K, weights)
        assert want["corners"].max() == R and want["corners"].min() == 0 and want["displacements"].any()


# ---- flavours and edits ---------------------------------------------------------------------------------------------------------------------------------------
def test_flavours_of_a_triangle_build(mv):
    v = bunny_tris().reshape(-1, 3)
    lo = v.min(0)
    dps = np.float32((v.max(0) - lo).max() / np.float32(64))
    B = mv.IntersectorOctreeGPU
    flavours = set()
    for flags in (0, B.BUILD_NO_DAG, B.BUILD_NO_EMBEDDED_MASK, B.BUILD_NO_DAG | B.BUILD_NO_EMBEDDED_MASK, B.BUILD_CONSERVATIVE):
        svo = mv.IntersectorOctreeGPU()
        svo.build(v, None, None, None, lo, dps, 64, flags=flags)
        xyz, _ = svo.read_voxels()
        check(mv, xyz, 64, 3, svo=svo, lower=lo, dps=dps)
        flavours.add(svo.info().flavour)
    assert len(flavours) > 1


def test_after_an_edit(mv):
    xyz, _ = block_and_noise(3, 32)
    svo = build(mv, xyz, 32)
    gone, fresh = xyz[::7], np.array([(0, 0, 0), (31, 31, 31), (7, 8, 8)], np.uint32)
    svo.edit_voxels(np.concatenate([gone, fresh]).astype(np.uint32), None, np.concatenate([np.zeros(len(gone), np.uint8), np.ones(len(fresh), np.uint8)]))
    keep = {tuple(p) for p in xyz.tolist()} - {tuple(p) for p in gone.tolist()} | {tuple(p) for p in fresh.tolist()}
    check(mv, np.array(sorted(keep)), 32, 2, svo=svo)


# ---- the contract of the call ---------------------------------------------------------------------------------------------------------------------------------
def params(mv, K=4, weights=(256, 256), limit=127):
    p = mv.SmoothParams()
    assert mv.lib().mvrt_smooth_default_params(C.byref(p)) == 0
    assert (p.iterations, p.weightEven, p.weightOdd, p.limit, list(p.reserved)) == (4, 256, 256, 127, [0] * 4)
    p.iterations, p.weightEven, p.weightOdd, p.limit = K, weights[0], weights[1], limit
    return p


def test_sizing_call_and_null_outputs(mv, ball16):
    want = M.smooth(M.ball(16, 6.3), 16, LOWER, DPS)
    n, m = len(want["faceVoxel"]), len(want["corners"])
    assert ball16.surface_smooth_device() == (n, m, 0)  # no iteration ran
    assert mv.lib().mvrt_svo_surface_smooth(ball16._h, None, None, 0, 0, None, None, None, None, None, None, None, None, None, None) == 0  # the counts may be NULL too
    disp = mv.DeviceArray((m, 3), np.int32)
    assert ball16.surface_smooth_device(None, 0, m, displacements=disp) == (n, m, want["clamped"])  # NULL params: the defaults; no face array: their capacity is not looked at
    assert np.array_equal(disp.to_host(), want["displacements"])
    fv = mv.DeviceArray(n, np.uint32)
    assert ball16.surface_smooth_device(params(mv), n, 0, faceVoxel=fv) == (n, m, want["clamped"]) and np.array_equal(fv.to_host(), want["faceVoxel"])
    vtx, nbr = mv.DeviceArray((m + 3, 3), np.float32), mv.DeviceArray(m + 3, np.uint8)  # a larger capacity writes the count's worth
    ball16.surface_smooth_device(params(mv), 0, m + 3, vertices=vtx, neighbours=nbr)
    assert np.array_equal(bits(vtx.to_host()[:m]), bits(want["vertices"])) and np.array_equal(nbr.to_host()[:m], want["neighbours"])


def test_capacity_one_short(mv, ball16):
    want = M.smooth(M.ball(16, 6.3), 16, LOWER, DPS)
    n, m = len(want["faceVoxel"]), len(want["corners"])
    outs = [filled(mv, s, t) for s, t in ((n, np.uint32), (n, np.uint8), ((n, 4), np.uint32), ((m, 3), np.float32), ((m, 3), np.int32), (m, np.uint8))]
    ptrs = [d.ptr for d, _ in outs]
    lib = mv.lib()
    for caps, what, count in (((n - 1, m), b"faceCapacity", b"%d faces" % n), ((n, m - 1), b"vertexCapacity", b"%d vertices" % m)):
        nf, nv, cl = C.c_uint64(0), C.c_uint64(0), C.c_uint64(9)
        assert lib.mvrt_svo_surface_smooth(ball16._h, None, None, caps[0], caps[1], *ptrs, C.byref(nf), C.byref(nv), C.byref(cl), None) != 0
        assert (nf.value, nv.value, cl.value) == (n, m, 0) and what in lib.mvrt_last_error() and count in lib.mvrt_last_error()
        for k in range(3, 6):  # ... and with a single vertex array
            if what == b"vertexCapacity":
                one = [None] * 6
                one[k] = ptrs[k]
                assert lib.mvrt_svo_surface_smooth(ball16._h, None, None, 0, m - 1, *one, None, None, None, None) != 0 and what in lib.mvrt_last_error()
    for dev, host in outs:
        assert np.array_equal(dev.to_host().view(np.uint8), host.view(np.uint8))  # nothing was written


def test_refusals_without_gpu_work(mv, ball16):
    empty = mv.IntersectorOctreeGPU()
    nodes, attrs, _ = ball16.download()
    i = ball16.info()
    up = mv.IntersectorOctreeGPU()
    up.upload(nodes, attrs, LOWER, DPS, 16, i.hasEmission, embeddedMask=bool(i.embeddedMask))
    before = mv.allocation_state()[2]
    for h, text in ((empty, "no octree"), (up, "keeps no Morton codes")):
        for call in (h.surface_smooth_device, h.surface_smooth):
            with pytest.raises(mv.MvrtError, match=text):
                call()
    for field, value in (("iterations", 257), ("weightOdd", -257), ("limit", 129)):
        p = params(mv)
        setattr(p, field, value)
        with pytest.raises(mv.MvrtError, match=field):
            ball16.surface_smooth_device(p)
    assert mv.allocation_state()[2] == before


def test_the_handle_is_not_modified(mv, ball16):
    before, info = ball16.download(want_morton=True), bytes(ball16.info())
    held = mv.allocation_state()[:2]
    ball16.surface_smooth(5, TAUBIN)
    ball16.surface_smooth(2, masks=np.full(ball16.info().numberOfVoxels, 0x2A, np.uint8))
    assert all(np.array_equal(a, b) for a, b in zip(ball16.download(want_morton=True), before)) and bytes(ball16.info()) == info
    assert mv.allocation_state()[:2] == held  # the scratch is gone
