"""apps/voxel_mesh --recolour-from and --distance-to on the bunny at 64^3 against a second model, the bunny mirrored and shifted with other colours, written here:
the printed counts and the face colours of the PLY equal the same sequence through the Python wrapper (build both on the joint grid, transfer_attributes or
nearest_between, the surface model on the voxels read back).  And the option conflicts."""
import math
import os
import subprocess

import numpy as np
import pytest

import surface_expected as S
from common import bunny_tris, position_colors
from voxel_mesh_app import APP, run, write_obj

pytestmark = pytest.mark.gpu

RES = 64


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    from massivevoxelraytracing_amd import build as b
    b.build_apps(verbose=False)
    d = tmp_path_factory.mktemp("query_app")
    tris = bunny_tris()
    v = tris.reshape(-1, 3).astype(np.float32)
    c = np.asarray(position_colors(tris)[0], np.float32).reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    w = v.copy()
    w[:, 0] = lo[0] + hi[0] - w[:, 0]  # mirrored in x
    w = (w + (hi - lo) * np.array([0.1, 0.05, -0.05], np.float32)).astype(np.float32)  # and shifted
    c2 = np.ascontiguousarray(c[:, ::-1])  # other colours
    return write_obj(d / "bunny.obj", v, c), write_obj(d / "other.obj", w, c2), (v, w, c, c2)


def both(mv, scene):
    _, _, (v, w, c, c2) = scene
    joint = np.concatenate([v, w])
    origin = joint.min(0)
    dps = np.float32((joint.max(0) - origin).max() / np.float32(RES))
    a, b = mv.IntersectorOctreeGPU(), mv.IntersectorOctreeGPU()
    a.build(v, c, None, None, origin, dps, RES)
    b.build(w, c2, None, None, origin, dps, RES)
    return a, b, origin, dps


def assert_ply(svo, origin, dps, ply, out):
    xyz, attrs = svo.read_voxels()
    want = S.surface(xyz, RES, origin, dps)
    vertices, indices, colours = S.read_ply_quads(str(ply))
    assert len(indices) == want["nFaces"] and "voxels %d faces %d vertices %d" % (len(xyz), len(indices), len(vertices)) in out
    assert np.array_equal(np.ascontiguousarray(vertices).view(np.uint32), want["vertices"].view(np.uint32)) and np.array_equal(indices, want["indices"])
    assert np.array_equal(colours, attrs[want["faceVoxel"], :3])


@pytest.mark.parametrize("limit", [None, 2])
def test_recolour_from_equals_the_python_route(tmp_path, scene, limit):
    import massivevoxelraytracing_amd as mv
    bunny, other, _ = scene
    offset = (1, 0, -2)
    out = run(bunny, RES, tmp_path / "out.ply", "--recolour-from", other, "--offset", *offset, *([] if limit is None else ["--recolour-max", limit]))
    a, b, origin, dps = both(mv, scene)
    before = a.read_voxels()[1]
    changed, beyond = a.transfer_attributes(b, offset, mv.NO_LIMIT if limit is None else limit * limit)
    n = a.info().numberOfVoxels
    assert "recolour-from: voxels %d, other %d, offset 1 0 -2, max %d, changed %d, beyond %d\n" % (n, b.info().numberOfVoxels, -1 if limit is None else limit, changed, beyond) in out
    assert changed > 1000 and (beyond == 0 if limit is None else 0 < beyond < n) and (a.read_voxels()[1] != before).any(1).sum() == changed
    assert_ply(a, origin, dps, tmp_path / "out.ply", out)


def test_distance_to_equals_the_python_route(tmp_path, scene):
    import massivevoxelraytracing_amd as mv
    bunny, other, _ = scene
    out = run(bunny, RES, tmp_path / "out.ply", "--distance-to", other, "--offset", 0, 3, 0)
    a, b, origin, dps = both(mv, scene)
    parts = []
    for name, r, xyz in (("a -> b", a.nearest_between_device(b, (0, 3, 0)), a.read_voxels()[0]), ("b -> a", b.nearest_between_device(a, (0, -3, 0)), b.read_voxels()[0])):
        parts.append("; %s: max %.6f (d2 %d) at voxel %d (%d %d %d), zero %d of %d" % ((name, math.sqrt(r["maxDist2"]), r["maxDist2"], r["farthest"]) + tuple(xyz[r["farthest"]]) +
                                                                                       (r["zero"], r["n"])))
        assert r["maxDist2"] > 4
    assert "distance-to: offset 0 3 0" + parts[0] + parts[1] + "\n" in out
    assert_ply(a, origin, dps, tmp_path / "out.ply", out)  # the mesh is written as without the flag


@pytest.mark.parametrize("options", [["--recolour-from", "O", "--union", "O"], ["--distance-to", "O", "--recolour-from", "O"], ["--distance-to", "O", "--xor", "O"],
                                     ["--recolour-max", "3"], ["--distance-to", "O", "--recolour-max", "3"], ["--recolour-from", "O", "--recolour-max", "-2"]])
def test_option_conflicts(tmp_path, scene, options):
    r = subprocess.run([APP, scene[0], str(RES), str(tmp_path / "no.ply")] + [scene[1] if o == "O" else o for o in options], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--recolour" in r.stderr and not os.path.exists(tmp_path / "no.ply")
