"""apps/voxel_mesh --union other.obj --rotate-b ax ay az deg [--scale-b s] on golden meshes: the bunny joined with a second bunny turned about the grid centre.
The printed counts equal those of the Python route -- both meshes voxelised on the joint lattice, the second resampled with the transform
cell_transform_from_world makes of the same world matrix, the model of tests/combine_expected.py on the two lists -- and the PLY holds the faces
tests/surface_expected.py finds on that set.  And the refusals of the new options: without one of the four operators, and a scale of 0."""
import os
import re
import subprocess

import numpy as np
import pytest

import combine_expected as CE
import resample_expected as E
import surface_expected as S
from common import bunny_tris
from voxel_mesh_app import APP, run, write_obj

pytestmark = pytest.mark.gpu

RES = 64


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """(first.obj, other.obj, origin, dps, the voxels and attributes of both on the joint lattice): the bunny, and the bunny mirrored in x and moved up a little,
    so that the two sets differ and the joint box is larger than either"""
    import massivevoxelraytracing_amd as mv
    from massivevoxelraytracing_amd import build as b
    b.build_apps(verbose=False)
    d = tmp_path_factory.mktemp("resample_app")
    first = bunny_tris().reshape(-1, 3).astype(np.float32)
    other = first.copy()
    other[:, 0] = first[:, 0].max() + first[:, 0].min() - other[:, 0]
    other[:, 1] += np.float32(0.1) * (first[:, 1].max() - first[:, 1].min())
    joint = np.concatenate([first, other])
    origin = joint.min(0)
    dps = np.float32((joint.max(0) - origin).max() / np.float32(RES))
    handles = []
    for v in (first, other):
        svo = mv.IntersectorOctreeGPU()
        svo.build(v, None, None, None, origin, dps, RES)
        handles.append(svo)
    return write_obj(d / "first.obj", first), write_obj(d / "other.obj", other), origin, dps, handles


def world_about_centre(origin, dps, axis, degrees, scale):
    """p' = s R ( p - centre ) + centre with the centre of the grid, as the app builds it: 3x4 row-major"""
    half = 0.5 * float(dps) * RES
    centre = origin.astype(np.float64) + half
    W = scale * E.rotation(axis, degrees)
    return np.concatenate([W, (centre - W @ centre).reshape(3, 1)], 1)


@pytest.mark.parametrize("axis,degrees,scale,offset", [((0, 0, 1), 90.0, None, None), ((1, 2, 3), 30.0, 0.75, (2, 0, -1))])
def test_union_with_the_turned_second_model_against_the_python_route(tmp_path, scene, axis, degrees, scale, offset):
    import massivevoxelraytracing_amd as mv
    first, other, origin, dps, (a, b) = scene
    xf = mv.cell_transform_from_world(world_about_centre(origin, dps, axis, degrees, 1.0 if scale is None else scale), origin, dps, origin, dps)
    turned = b.resample(xf, mv.IntersectorOctreeGPU())
    (xa, aa), (xb, ab), (xt, at) = a.read_voxels(), b.read_voxels(), turned.read_voxels()
    model = E.dense(xb, ab, RES, *xf.arrays(), RES)
    assert np.array_equal(xt, model["xyz"]) and np.array_equal(at, model["attribs"]) and 0 < len(xt) and not np.array_equal(xt, xb)
    want = CE.combine(xa, aa, xt, at, RES, CE.UNION, offset)
    ply = tmp_path / "out.ply"
    out = run(first, RES, ply, "--union", other, "--rotate-b", *axis, degrees, *(["--scale-b", scale] if scale else []), *((["--offset"] + list(offset)) if offset else []))
    m = re.search(r"^resample-b: voxels (\d+) -> (\d+), axis", out, re.M)
    assert m and [int(x) for x in m.groups()] == [len(xb), len(xt)]  # the second set's voxels before / after
    m = re.search(r"^union: voxels (\d+) -> (\d+), other (\d+), offset (-?\d+) (-?\d+) (-?\d+), overlap (\d+), clipped (\d+), added (\d+), removed (\d+)$", out, re.M)
    assert m and [int(x) for x in m.groups()] == [len(xa), len(want["xyz"]), len(xt)] + list(offset or (0, 0, 0)) + [want["overlap"], want["clipped"], len(want["xyz"]) - len(xa), 0]
    assert out.index("resample-b:") < out.index("union:")
    voxels = S.sorted_voxels(want["xyz"])
    face_voxel = S.faces(voxels, S.masks_of(voxels, RES))[0]
    vertices, indices, colours = S.read_ply_quads(str(ply))
    assert "voxels %d faces %d " % (len(voxels), len(face_voxel)) in out and len(indices) == len(face_voxel) > 0
    assert np.array_equal(colours, want["attribs"][face_voxel][:, :3])


def test_the_new_options_are_refused_without_an_operator_and_with_scale_zero(tmp_path, scene):
    first, other = scene[:2]
    for args in (["--rotate-b", "0", "0", "1", "90"], ["--scale-b", "2"], ["--union", other, "--scale-b", "0"], ["--union", other, "--scale-b", "-1"],
                 ["--union", other, "--rotate-b", "0", "0", "0", "90"]):
        r = subprocess.run([APP, first, str(RES), str(tmp_path / "no.ply")] + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--rotate-b" in r.stderr and "--scale-b" in r.stderr and not os.path.exists(tmp_path / "no.ply")
