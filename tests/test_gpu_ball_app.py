"""apps/voxel_mesh --round-close 5 --fill on a box with a hole in its floor, written here as an OBJ: the fill alone finds no enclosed cell; behind the closing
with the ball of 5 it fills the inside.  The printed counts equal those of the Python calls on the same build.  And the C++ mirror's round-offset methods,
compiled and run (tests/cpp/ball_usage.cpp)."""
import os
import re
import subprocess

import numpy as np
import pytest

import ball_expected as B
import common
import surface_expected as S
from voxel_mesh_app import APP, holed_box, write_obj

pytestmark = pytest.mark.gpu

RES = 16


@pytest.fixture(scope="module")
def box_obj(tmp_path_factory):
    from massivevoxelraytracing_amd import build as b
    b.build_apps(verbose=False)
    tris = holed_box()
    path = tmp_path_factory.mktemp("ball_app") / "box.obj"
    return write_obj(path, tris), tris


def built(mv, tris):
    v = tris.reshape(-1, 3)
    lo = v.min(0)
    svo = mv.IntersectorOctreeGPU()
    svo.build(v, None, None, None, lo, np.float32((v.max(0) - lo).max() / np.float32(RES)), RES)
    return svo


def test_round_close_then_fill_repairs_the_leaky_box(tmp_path, box_obj):
    import massivevoxelraytracing_amd as mv
    obj, tris = box_obj
    svo = built(mv, tris)
    n0 = svo.info().numberOfVoxels
    x0, a0 = svo.read_voxels()
    assert svo.enclosed_cells_device() == (0, 0)  # the hole makes the whole inside exterior
    added = svo.close_ball(5)
    n1 = svo.info().numberOfVoxels
    assert added == n1 - n0 > 0 and np.array_equal(svo.read_voxels()[0], B.ball("close", x0, a0, RES, 5)[0])
    cells, regions = svo.enclosed_cells_device()
    assert cells > 1000 and regions == 1
    assert svo.fill_enclosed() == cells
    out = subprocess.check_output([APP, obj, str(RES), str(tmp_path / "closed.ply"), "--round-close", "5", "--fill"], timeout=120).decode()
    print(out)
    assert "round-close: voxels %d -> %d, radius2 5, added %d" % (n0, n1, added) in out
    assert "fill: voxels %d -> %d, enclosed cells %d in 1 regions, filled %d" % (n1, n1 + cells, cells, cells) in out
    assert out.index("round-close:") < out.index("fill:")
    masks, nfaces = svo.surface_masks()
    assert re.search(r"voxels %d faces %d " % (n1 + cells, nfaces), out)
    assert len(S.read_ply_quads(tmp_path / "closed.ply")[1]) == nfaces


def test_the_other_operators_and_the_refused_combinations(tmp_path, box_obj):
    import massivevoxelraytracing_amd as mv
    obj, tris = box_obj
    svo = built(mv, tris)
    n0 = svo.info().numberOfVoxels
    changed = svo.dilate_ball(9)
    out = subprocess.check_output([APP, obj, str(RES), str(tmp_path / "op.ply"), "--round-dilate", "9"], timeout=120).decode()
    print(out)
    assert "round-dilate: voxels %d -> %d, radius2 9, added %d" % (n0, svo.info().numberOfVoxels, changed) in out
    for flags in (["--round-close", "5", "--round-open", "5"], ["--round-close", "0"], ["--round-close", "1025"], ["--round-close", "5", "--close", "1"]):
        r = subprocess.run([APP, obj, str(RES), str(tmp_path / "no.ply")] + flags, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--round-dilate / --round-erode / --round-close / --round-open" in r.stderr and not os.path.exists(tmp_path / "no.ply")


def test_cpp_mirror_runs(tmp_path):
    exe, _ = common.compile_usage(tmp_path, "ball_usage")
    out = subprocess.check_output([str(exe), "run"], timeout=120).decode()
    print(out)
    assert "shell 217 cells 485 farthest 3 thin 217 deepest 1 plugged 1 enclosed 125 grown 392 opened 0 eroded 348 left 262" in out
