"""Per-face ambient occlusion on the MI355X: mvrt_svo_surface_ao counts, per exposed face, the Hammersley / sampleLambertian shadow rays that leave the face
centre unoccluded within the radius.  Expected values are the CPU oracle's trace of the same ray bits (origins rebuilt in fp32 exactly as mvrt.h states them,
directions from mvrt_ao_directions, which tests/test_range_cpu.py compares with the oracle), filtered by t <= radius; all comparisons are exact."""
import os
import subprocess

import numpy as np
import pytest

import common
import surface_expected as S
from common import bunny_tris, position_colors
from fixtures import mv, O  # noqa: F401 (fixtures)
from rays import AXIS, PLUS, expected_open, oracle_t

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXF = np.float32(3.402823466e38)


def voxel_scene(O, xyz, res, origin, dps):
    """the oracle's octree over a voxel list (white, no emission)"""
    m = np.unique(O.morton_encode_batch(np.asarray(xyz, np.uint32)))
    attrs = np.zeros((len(m), 8), np.uint8)
    attrs[:, :4] = 255
    return O.Scene(O.build_octree(m, res), attrs, origin, dps, res)


@pytest.fixture(scope="module")
def bunny(mv, O):
    """per grid resolution: the oracle scene and, per sample count, the oracle's t of the bake's rays -- computed once, shared, never modified"""
    from massivevoxelraytracing_amd import scenes
    cache = {}

    def get(res, K, flags=0):
        tris = bunny_tris()
        v = tris.reshape(-1, 3)
        if res not in cache:
            cache[res] = {"sc": O.build_scene_from_triangles(tris, res)}
        c = cache[res]
        origin, dps = scenes.bounding_grid(v, res)
        svo = mv.IntersectorOctreeGPU()
        svo.build(v, None, None, None, origin, dps, res, flags=flags)
        xyz, _ = svo.read_voxels()
        q = svo.surface_quads()
        if ("t", K) not in c:
            c["faces"] = (q["faceVoxel"].copy(), q["faceDir"].copy())
            c[("t", K)] = oracle_t(mv, c["sc"], xyz, q["faceVoxel"], q["faceDir"], K)
            c[("t", K)].setflags(write=False)
        assert np.array_equal(c["faces"][0], q["faceVoxel"]) and np.array_equal(c["faces"][1], q["faceDir"])  # every flavour lists the same faces
        return svo, q, c[("t", K)]
    return get


def test_bunny_64(mv, bunny):
    svo, q, t = bunny(64, 64)
    dps = np.float32(svo.info().dps)
    n = len(q["faceVoxel"])
    assert n > 5000
    for radius in (np.float32(0.25) * dps, np.float32(8) * dps, MAXF):
        got = svo.surface_ao(64, radius)
        assert np.array_equal(got["faceVoxel"], q["faceVoxel"]) and np.array_equal(got["faceDir"], q["faceDir"])
        want = expected_open(t, radius)
        assert np.array_equal(got["open"], want), radius
        if radius == np.float32(8) * dps:
            assert not (want == 0).all() and not (want == 64).all() and len(np.unique(want)) > 8
    assert np.array_equal(svo.surface_ao()["open"], expected_open(t, np.float32(8) * dps))  # the defaults: 64 samples, 8 voxels
    assert np.array_equal(svo.surface_ao(64, np.inf)["open"], expected_open(t, MAXF))


@pytest.mark.parametrize("flags", [0, 2])
@pytest.mark.parametrize("K", [1, 16, 256])
def test_bunny_32(mv, bunny, K, flags):
    svo, q, t = bunny(32, K, flags)
    assert svo.info().flavour == (1 if flags & 2 else 0)
    dps = np.float32(svo.info().dps)
    for radius in (np.float32(2) * dps, np.float32(8) * dps):
        assert np.array_equal(svo.surface_ao(K, radius)["open"], expected_open(t, radius)), radius


def build_set(mv, xyz, res=8, dps=0.125, origin=(-0.5, 0.25, 1.0)):
    svo = mv.IntersectorOctreeGPU()
    svo.build_voxels(np.asarray(xyz, np.uint32), None, origin=origin, dps=dps, gridRes=res)
    return svo


def test_single_voxel_is_open_at_any_radius(mv):
    svo = build_set(mv, [(3, 4, 5)])
    for K in (1, 16, 64, 256):
        for radius in (0.01, 0.125, 1.0, MAXF):
            a = svo.surface_ao(K, radius)
            assert a["faceDir"].tolist() == [0, 1, 2, 3, 4, 5] and (a["open"] == K).all()


def test_two_voxels_two_cells_apart(mv, O):
    xyz = [(2, 4, 4), (5, 4, 4)]
    svo = build_set(mv, xyz)
    near, far = svo.surface_ao(64, 0.125), svo.surface_ao(64, MAXF)
    assert len(near["open"]) == 12 and (near["open"] == 64).all()  # the gap is two voxels wide, the radius one
    facing = ((far["faceVoxel"] == 0) & (far["faceDir"] == 3)) | ((far["faceVoxel"] == 1) & (far["faceDir"] == 5))
    assert facing.sum() == 2 and (far["open"][facing] < 64).all() and (far["open"][facing] > 0).all() and (far["open"][~facing] == 64).all()
    sc = voxel_scene(O, xyz, 8, np.array((-0.5, 0.25, 1.0), np.float32), 0.125)
    t = oracle_t(mv, sc, svo.read_voxels()[0], far["faceVoxel"], far["faceDir"], 64)
    assert np.array_equal(far["open"], expected_open(t, MAXF)) and np.array_equal(svo.surface_ao(64, 0.375)["open"], expected_open(t, 0.375))


def test_hollow_shell_inner_faces_are_open_within_a_quarter_voxel(mv, O):
    g = np.argwhere(np.ones((6, 6, 6), bool)) + 1
    shell = g[((g == 1) | (g == 6)).any(1)]
    svo = build_set(mv, shell)
    a = svo.surface_ao(64, np.float32(0.25) * np.float32(0.125))
    xyz = svo.read_voxels()[0]
    # inner faces: the neighbour cell in the face's direction lies inside the shell's hollow
    nb = xyz[a["faceVoxel"]].astype(np.int64)
    nb[np.arange(len(nb)), AXIS[a["faceDir"]]] += np.where(PLUS[a["faceDir"]] == 1, 1, -1)
    inner = ((nb >= 2) & (nb <= 5)).all(1)
    assert inner.sum() == 6 * 16 and (a["open"][inner] == 64).all() and (a["open"] == 64).all()
    sc = voxel_scene(O, shell, 8, np.array((-0.5, 0.25, 1.0), np.float32), 0.125)
    t = oracle_t(mv, sc, xyz, a["faceVoxel"], a["faceDir"], 64)
    far = svo.surface_ao(64, MAXF)["open"]
    assert np.array_equal(far, expected_open(t, MAXF)) and (far[inner] == 0).all()  # the hollow is closed: no inner ray reaches the sky


def test_out_of_range_entries_are_refused_before_anything_is_written(mv):
    rng = np.random.default_rng(5)
    svo = build_set(mv, np.argwhere(rng.random((8, 8, 8)) < 0.3))
    nv = svo.info().numberOfVoxels
    q = svo.surface_quads()
    n = len(q["faceVoxel"])
    assert n > 300
    sentinel = np.full(n, 0xA5A5, np.uint16)
    for bad_voxel, bad_dir, lowest in (((200, nv), None, 200), (None, (100, 6), 100), ((250, nv), (17, 6), 17), ((3, 0xFFFFFFFF), (3, 255), 3), ((n - 1, nv), None, n - 1)):
        fv, fd = q["faceVoxel"].copy(), q["faceDir"].copy()
        if bad_voxel:
            fv[bad_voxel[0]] = bad_voxel[1]
        if bad_dir:
            fd[bad_dir[0]] = bad_dir[1]
        out = mv.DeviceArray.from_host(sentinel)
        with pytest.raises(mv.MvrtError, match=r"entry %d is out of range" % lowest):
            svo.surface_ao_device(n, mv.DeviceArray.from_host(fv), mv.DeviceArray.from_host(fd), 16, 1.0, out)
        assert np.array_equal(out.to_host(), sentinel)
    # any list of (vIndex, direction) pairs is legal: faces that are not exposed, repeated, in any order
    fv, fd = np.array([5, 5, 0, nv - 1], np.uint32), np.array([0, 0, 5, 3], np.uint8)
    out = mv.DeviceArray.from_host(sentinel[:4])
    svo.surface_ao_device(4, mv.DeviceArray.from_host(fv), mv.DeviceArray.from_host(fd), 16, 1.0, out)
    got = out.to_host()
    assert got[0] == got[1] and (got <= 16).all()
    svo.surface_ao_device(0, None, None, 16, 1.0, None)  # no faces: nothing to do


def test_uploaded_and_empty_handles_are_refused(mv, O):
    sc = O.build_scene_from_triangles(bunny_tris(), 16)
    svo = mv.IntersectorOctreeGPU()
    one = mv.DeviceArray(4, np.uint32)
    with pytest.raises(mv.MvrtError, match="no octree"):
        svo.surface_ao_device(1, one, one, 16, 1.0, one)
    svo.upload(sc.nodes, sc.attrs, sc.origin, sc.dps, sc.grid_res, sc.has_emission)
    with pytest.raises(mv.MvrtError, match="keeps no Morton codes"):
        svo.surface_ao_device(1, one, one, 16, 1.0, one)
    svo.rebuild()
    assert (svo.surface_ao(16)["open"] <= 16).all()


def test_cpp_mirror_range_methods_run(tmp_path, mv):
    exe, libdir = common.compile_usage(tmp_path, "range_usage", missing=None)
    r = subprocess.run(["timeout", "-k", "10", "120", str(exe), "run"], capture_output=True, text=True)
    assert r.returncode == 0 and "faces 12 nearAll 12 farLess 2 t 3 3.40282347e+38" in r.stdout, (r.returncode, r.stdout, r.stderr)


def run_voxel_mesh(args):
    return subprocess.run(["timeout", "-k", "10", "120", os.path.join(ROOT, "apps", "voxel_mesh")] + args, capture_output=True, text=True)


@pytest.mark.parametrize("weld", [True, False])
def test_voxel_mesh_app_bakes_the_occlusion_into_the_colours(tmp_path, mv, weld):
    from massivevoxelraytracing_amd import build as b
    b.build_apps(verbose=False)
    tris = bunny_tris()
    v = tris.reshape(-1, 3)
    cols = position_colors(tris)[0].reshape(-1, 3)
    obj = str(tmp_path / "bunny.obj")
    with open(obj, "w") as f:
        f.write("".join("v %.9g %.9g %.9g %.9g %.9g %.9g\n" % (*p, *c) for p, c in zip(v, cols)) + "".join("f %d %d %d\n" % (3 * t + 1, 3 * t + 2, 3 * t + 3) for t in range(len(tris))))
    extra = [] if weld else ["--no-weld"]
    plain, baked = str(tmp_path / "plain.ply"), str(tmp_path / "baked.ply")
    r0, r1 = run_voxel_mesh([obj, "64", plain] + extra), run_voxel_mesh([obj, "64", baked, "--ao", "16"] + extra)
    assert r0.returncode == 0 and r1.returncode == 0, r0.stderr + r1.stderr
    assert r0.stdout.replace("plain.ply", "") == r1.stdout.replace("baked.ply", "")  # the same counts
    v0, i0, c0 = S.read_ply_quads(plain)
    v1, i1, c1 = S.read_ply_quads(baked)
    assert np.array_equal(v0.view(np.uint32), v1.view(np.uint32)) and np.array_equal(i0, i1)
    head = lambda p: open(p, "rb").read().split(b"end_header")[0]
    assert head(plain) == head(baked)
    lo = v.min(0)
    svo = mv.IntersectorOctreeGPU()
    svo.build(v, cols, None, None, lo, np.float32((v.max(0) - lo).max() / np.float32(64)), 64)
    a = svo.surface_ao(16)
    _, attrs = svo.read_voxels()
    assert np.array_equal(c0, attrs[a["faceVoxel"], :3]) and len(np.unique(c0)) > 16
    want = ((c0.astype(np.uint32) * a["open"].astype(np.uint32)[:, None] + 8) // 16).astype(np.uint8)
    assert np.array_equal(c1, want) and not np.array_equal(c1, c0)


def test_voxel_mesh_app_refuses_ao_with_merge(tmp_path):
    for flag in ("--merge", "--merge-any"):
        r = run_voxel_mesh([str(tmp_path / "none.obj"), "64", str(tmp_path / "out.ply"), "--ao", flag])
        assert r.returncode not in (0, 124, 137) and "--ao cannot be combined with --merge" in r.stderr
