"""apps/voxel_mesh --exterior: the bunny at 64^3 without the inner side of its shell, the octree left as built.  The PLY equals that of --fill face for face:
a filled voxel owns no face, so the faces, their order, the welded vertices and the colours are the same; the report line names the faces before and after.
And the C++ mirror's exterior and masked methods, compiled and run (tests/cpp/exterior_usage.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import common
import surface_expected as S
from common import bunny_tris
from voxel_mesh_app import APP, write_obj

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bunny_obj(tmp_path_factory):
    from massivevoxelraytracing_amd import build as b
    b.build_apps(verbose=False)
    tris = bunny_tris()
    return write_obj(tmp_path_factory.mktemp("exterior_app") / "bunny.obj", tris)


def run(obj, ply, *flags):
    return subprocess.check_output([APP, obj, "64", str(ply)] + list(flags), timeout=120).decode()


@pytest.mark.parametrize("extra", [[], ["--no-weld"], ["--merge"], ["--merge-any", "--no-weld"]])
def test_exterior_ply_equals_the_fill_ply(tmp_path, bunny_obj, extra):
    out = run(bunny_obj, tmp_path / "exterior.ply", "--exterior", *extra)
    run(bunny_obj, tmp_path / "fill.ply", "--fill", *extra)
    print(out)
    assert "exterior: faces 27550 -> 14558, 12992 look into an enclosed cell" in out
    assert "voxels 8516 faces 14558 " in out  # the octree is the one the build left
    ve, ie, ce = S.read_ply_quads(tmp_path / "exterior.ply")
    vf, jf, cf = S.read_ply_quads(tmp_path / "fill.ply")
    if "--merge" not in extra and "--merge-any" not in extra:
        assert len(ie) == 14558
    else:
        assert len(ie) < 14558 and "rects %d" % len(ie) in out
    assert np.array_equal(np.ascontiguousarray(ve).view(np.uint32), np.ascontiguousarray(vf).view(np.uint32)) and np.array_equal(ie, jf) and np.array_equal(ce, cf)


def test_exterior_with_ao_runs(tmp_path, bunny_obj):
    out = run(bunny_obj, tmp_path / "ao.ply", "--exterior", "--ao", "16")
    assert "faces 14558 " in out
    _, indices, colours = S.read_ply_quads(tmp_path / "ao.ply")
    assert len(indices) == 14558 and len(colours) == 14558 and len(np.unique(colours)) > 4  # white voxels, shaded by the bake


def test_exterior_with_fill_is_refused(tmp_path, bunny_obj):
    r = subprocess.run([APP, bunny_obj, "64", str(tmp_path / "no.ply"), "--exterior", "--fill"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--exterior cannot be combined with --fill" in r.stderr and not os.path.exists(tmp_path / "no.ply")


def test_cpp_mirror_runs(tmp_path):
    import massivevoxelraytracing_amd as mv
    exe, libdir = common.compile_usage(tmp_path, "exterior_usage")
    out = subprocess.check_output([str(exe), "run"], timeout=120).decode()
    print(out)
    assert "plain 120 exterior 96 hidden 24 counts 96 24 quads 96 mesh 96 vertices 98 covered 96 rects 6 corners 8 same 1" in out
