"""apps/voxel_mesh --union / --intersect / --subtract / --xor other.obj [--offset x y z] [--attrib-b] on two meshes written here as OBJ: two solid blocks that
share a corner region.  The printed counts equal those of the model (tests/combine_expected.py) on the Python builds of the same two meshes over the joint bounding
box, and the PLY holds the faces tests/surface_expected.py finds on the model's set."""
import os
import re
import subprocess

import numpy as np
import pytest

import combine_expected as E
import surface_expected as S
from voxel_mesh_app import APP, block, run, write_obj

pytestmark = pytest.mark.gpu

RES = 32
OPTIONS = {"--union": E.UNION, "--intersect": E.INTERSECTION, "--subtract": E.DIFFERENCE, "--xor": E.XOR}


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """(first.obj, other.obj, the voxels and attributes of both on the joint lattice): the first mesh holds solid blocks at [4, 12)^3 and [24, 30)^3 and two
    small triangles that stretch the bounding box to [0, 32]^3; the second, a block at [8, 16)^3, lies inside it, so the joint box is the first's"""
    import massivevoxelraytracing_amd as mv
    from massivevoxelraytracing_amd import build as b
    b.build_apps(verbose=False)
    d = tmp_path_factory.mktemp("combine_app")
    lo, hi, e = 0.0, 32.0, 0.4
    first = np.array([(lo, lo, lo), (lo + e, lo, lo), (lo, lo + e, lo), (hi, hi, hi), (hi - e, hi, hi), (hi, hi - e, hi)] + block(4, 12) + block(24, 30), np.float32).reshape(-1, 3, 3)
    other = np.array(block(8, 16), np.float32).reshape(-1, 3, 3)
    joint = np.concatenate([first.reshape(-1, 3), other.reshape(-1, 3)])
    origin = joint.min(0)
    dps = np.float32((joint.max(0) - origin).max() / np.float32(RES))
    sets = []
    for tris in (first, other):
        svo = mv.IntersectorOctreeGPU()
        svo.build(tris.reshape(-1, 3), None, None, None, origin, dps, RES)
        sets.append(svo.read_voxels())
    assert len(sets[1][0]) == 512 and len(sets[0][0]) >= 512
    return write_obj(d / "first.obj", first), write_obj(d / "other.obj", other), sets


@pytest.mark.parametrize("option", sorted(OPTIONS))
@pytest.mark.parametrize("offset,attrib_b", [(None, False), ((16, 16, 20), True)])
def test_each_option_against_the_model(tmp_path, scene, option, offset, attrib_b):
    first, other, ((xa, aa), (xb, ab)) = scene
    want = E.combine(xa, aa, xb, ab, RES, OPTIONS[option], offset, E.ATTRIB_B if attrib_b else 0)
    _, _, _, (added, removed) = E.edit_lists(xa, aa, xb, ab, RES, OPTIONS[option], offset, E.ATTRIB_B if attrib_b else 0)
    ply = tmp_path / "out.ply"
    out = run(first, RES, ply, option, other, *((["--offset"] + list(offset)) if offset else []), *(["--attrib-b"] if attrib_b else []))
    m = re.search(r"^(\w+): voxels (\d+) -> (\d+), other (\d+), offset (-?\d+) (-?\d+) (-?\d+), overlap (\d+), clipped (\d+), added (\d+), removed (\d+)$", out, re.M)
    assert m and m.group(1) == option[2:]
    assert [int(x) for x in m.groups()[1:]] == [len(xa), len(want["xyz"]), len(xb)] + list(offset or (0, 0, 0)) + [want["overlap"], want["clipped"], added, removed]
    if offset is None:
        assert want["overlap"] == 64 and want["clipped"] == 0
    else:
        assert want["clipped"] == 4 * 8 * 8 and want["overlap"] >= 72  # z = 28 .. 35 of the moved block: four layers leave the grid, two meet the first model's upper block
    voxels = S.sorted_voxels(want["xyz"])  # (the model's order already)
    face_voxel = S.faces(voxels, S.masks_of(voxels, RES))[0]
    vertices, indices, colours = S.read_ply_quads(str(ply))
    assert "voxels %d faces %d " % (len(voxels), len(face_voxel)) in out and len(indices) == len(face_voxel) > 0
    # one colour per face from its voxel: under --attrib-b the shared cells show the second model's colour, which the model's attributes hold
    assert np.array_equal(colours, want["attribs"][face_voxel][:, :3])


def test_only_one_of_the_four(tmp_path, scene):
    first, other, _ = scene
    r = subprocess.run([APP, first, str(RES), str(tmp_path / "no.ply"), "--union", other, "--xor", other], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--union" in r.stderr and not os.path.exists(tmp_path / "no.ply")


def test_the_combination_comes_before_the_later_stages(tmp_path, scene):
    first, other, ((xa, aa), (xb, ab)) = scene
    want = E.combine(xa, aa, xb, ab, RES, E.UNION)
    out = run(first, RES, tmp_path / "lod.ply", "--union", other, "--lod", "1", "--components")
    assert "union: voxels %d -> %d," % (len(xa), len(want["xyz"])) in out and "lod: voxels %d -> " % len(want["xyz"]) in out
    assert out.index("union:") < out.index("lod:") < out.index("components:")
