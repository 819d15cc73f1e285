"""apps/voxel_mesh --fill-nearest and --solid on the bunny with per-vertex colours at 64^3.  --fill-nearest: the printed counts and the PLY equal the Python
route (build, fill_enclosed_nearest, the surface model on the voxels read back).  --solid --subtract other.obj, the other model being the bunny mirrored and
shifted, written here: the printed counts and the face colours equal the same sequence through the Python wrapper, and the cut runs through the filled inside --
faces of voxels the fill added, in the colour of their nearest shell voxel, not white.  And the option conflicts."""
import os
import re
import subprocess

import numpy as np
import pytest

import surface_expected as S
from common import bunny_tris, position_colors
from voxel_mesh_app import APP, run, write_obj

pytestmark = pytest.mark.gpu

RES = 64
LINE = r"^%s: voxels (\d+) -> (\d+), enclosed cells (\d+) in (\d+) regions, deepest d2 (\d+), filled (\d+)$"


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    from massivevoxelraytracing_amd import build as b
    b.build_apps(verbose=False)
    d = tmp_path_factory.mktemp("nearest_app")
    tris = bunny_tris()
    v = tris.reshape(-1, 3).astype(np.float32)
    c = np.asarray(position_colors(tris)[0], np.float32).reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    w = v.copy()
    w[:, 0] = lo[0] + hi[0] - w[:, 0]  # mirrored in x
    w = (w + (hi - lo) * np.array([0.35, 0.1, -0.05], np.float32)).astype(np.float32)  # and shifted
    return write_obj(d / "bunny.obj", v, c), write_obj(d / "other.obj", w, c), (v, w, c)


def grid(*meshes):
    joint = np.concatenate(meshes)
    origin = joint.min(0)
    return origin, np.float32((joint.max(0) - origin).max() / np.float32(RES))


def assert_ply(mv, svo, origin, dps, ply, out):
    """the PLY against the surface model on the voxels of the handle: faces and one colour per face from its voxel; -> (voxels, attributes, the voxel of every face)"""
    xyz, attrs = svo.read_voxels()
    want = S.surface(xyz, RES, origin, dps)
    vertices, indices, colours = S.read_ply_quads(str(ply))
    assert len(indices) == want["nFaces"] and "voxels %d faces %d vertices %d" % (len(xyz), len(indices), len(vertices)) in out
    assert np.array_equal(np.ascontiguousarray(vertices).view(np.uint32), want["vertices"].view(np.uint32)) and np.array_equal(indices, want["indices"])
    assert np.array_equal(colours, attrs[want["faceVoxel"], :3])
    return xyz, attrs, want["faceVoxel"]


def test_fill_nearest_equals_the_python_route(tmp_path, scene):
    import massivevoxelraytracing_amd as mv
    bunny, _, (v, _, c) = scene
    out = run(bunny, RES, tmp_path / "out.ply", "--fill-nearest")
    origin, dps = grid(v)
    svo = mv.IntersectorOctreeGPU()
    svo.build(v, c, None, None, origin, dps, RES)
    n = svo.info().numberOfVoxels
    cells, regions = svo.enclosed_nearest_device()
    assert svo.fill_enclosed_nearest() == cells == 48162 and (n, regions) == (8516, 3)  # the bunny's numbers (tests/test_fill_cpu.py)
    m = re.search(LINE % "fill-nearest", out, re.M)
    assert m and [int(x) for x in m.groups()] == [n, n + cells, cells, regions, mv.enclosed_nearest_stats()["deepest"], cells]
    assert_ply(mv, svo, origin, dps, tmp_path / "out.ply", out)


def test_solid_subtract_shows_the_shells_colours_on_the_cut(tmp_path, scene):
    import massivevoxelraytracing_amd as mv
    bunny, other, (v, w, c) = scene
    out = run(bunny, RES, tmp_path / "cut.ply", "--solid", "--subtract", other)
    origin, dps = grid(v, w)
    a, b = mv.IntersectorOctreeGPU(), mv.IntersectorOctreeGPU()
    a.build(v, c, None, None, origin, dps, RES)
    b.build(w, c, None, None, origin, dps, RES)
    n = a.info().numberOfVoxels
    shell = S.morton(a.read_voxels()[0])
    listing = a.enclosed_nearest()  # before the fill
    cells = len(listing["xyz"])
    assert a.fill_enclosed_nearest() == cells > 1000
    deepest = mv.enclosed_nearest_stats()["deepest"]
    m = re.search(LINE % "solid", out, re.M)
    assert m and [int(x) for x in m.groups()] == [n, n + cells, cells, listing["nRegions"], deepest, cells] and deepest == listing["dist2"].max()
    added, removed, _ = a.combine(b, mv.COMBINE_DIFFERENCE)
    assert "subtract: voxels %d -> %d, other %d," % (n + cells, a.info().numberOfVoxels, b.info().numberOfVoxels) in out and "removed %d" % removed in out
    assert out.index("solid:") < out.index("subtract:") and added == 0 and removed > 0
    xyz, attrs, face_voxel = assert_ply(mv, a, origin, dps, tmp_path / "cut.ply", out)
    # the cut faces: faces of voxels the fill added, each in the colour of its nearest shell voxel
    codes = S.morton(xyz)
    inside = ~np.isin(codes[face_voxel], shell)
    assert inside.sum() > 100
    row = {int(k): i for i, k in enumerate(S.morton(listing["xyz"]))}
    rows = np.array([row[int(k)] for k in codes[face_voxel][inside]], np.int64)
    _, _, colours = S.read_ply_quads(str(tmp_path / "cut.ply"))
    assert np.array_equal(colours[inside], listing["attribs"][rows, :3]) and not (colours[inside] == 255).all(1).any()
    assert len(np.unique(colours[inside], axis=0)) > 50  # not one flat slab


@pytest.mark.parametrize("options", [["--fill-nearest", "--fill"], ["--fill-nearest", "--exterior"], ["--exterior", "--fill", "--fill-nearest"]])
def test_option_conflicts(tmp_path, scene, options):
    r = subprocess.run([APP, scene[0], str(RES), str(tmp_path / "no.ply")] + options, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--fill" in r.stderr and not os.path.exists(tmp_path / "no.ply")
