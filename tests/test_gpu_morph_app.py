"""apps/voxel_mesh --close 1 --fill, the repair route for a leaky shell: a box with a hole in its floor, written here as an OBJ.  The fill alone finds no enclosed
cell; behind a one-step closing it fills the inside.  The printed counts equal those of the Python calls on the same build.  And the C++ mirror's morphology
methods, compiled and run (tests/cpp/morph_usage.cpp)."""
import os
import re
import subprocess

import numpy as np
import pytest

import common
import morph_expected as M
import surface_expected as S
from voxel_mesh_app import APP, holed_box, write_obj

pytestmark = pytest.mark.gpu

RES = 16


@pytest.fixture(scope="module")
def box_obj(tmp_path_factory):
    from massivevoxelraytracing_amd import build as b
    b.build_apps(verbose=False)
    tris = holed_box()
    path = tmp_path_factory.mktemp("morph_app") / "box.obj"
    return write_obj(path, tris), tris


def test_close_then_fill_repairs_the_leaky_box(tmp_path, box_obj):
    import massivevoxelraytracing_amd as mv
    obj, tris = box_obj
    v = tris.reshape(-1, 3)
    lo = v.min(0)
    svo = mv.IntersectorOctreeGPU()
    svo.build(v, None, None, None, lo, np.float32((v.max(0) - lo).max() / np.float32(RES)), RES)
    n0 = svo.info().numberOfVoxels
    x0, a0 = svo.read_voxels()
    floor = x0[x0[:, 2] == 0]
    assert len(floor) == 16 * 16 - 1 and not (floor[:, :2] == 7).all(1).any()  # one voxel is missing from the floor
    assert svo.enclosed_cells_device() == (0, 0)  # the hole makes the whole inside exterior
    leaky = subprocess.check_output([APP, obj, str(RES), str(tmp_path / "leaky.ply"), "--fill"], timeout=120).decode()
    print(leaky)
    assert "fill: voxels %d -> %d, enclosed cells 0 in 0 regions, filled 0" % (n0, n0) in leaky
    added = svo.close(mv.MORPH_CUBE, 1)
    n1 = svo.info().numberOfVoxels
    assert added == n1 - n0 > 0 and np.array_equal(svo.read_voxels()[0], M.morph("close", x0, a0, RES, M.CUBE, 1)[0])
    cells, regions = svo.enclosed_cells_device()
    assert cells > 1000 and regions == 1
    assert svo.fill_enclosed() == cells
    out = subprocess.check_output([APP, obj, str(RES), str(tmp_path / "closed.ply"), "--close", "1", "--fill"], timeout=120).decode()
    print(out)
    assert "close: voxels %d -> %d, element cube, steps 1, added %d" % (n0, n1, added) in out
    assert "fill: voxels %d -> %d, enclosed cells %d in 1 regions, filled %d" % (n1, n1 + cells, cells, cells) in out
    assert out.index("close:") < out.index("fill:")
    masks, nfaces = svo.surface_masks()
    assert re.search(r"voxels %d faces %d " % (n1 + cells, nfaces), out)
    assert len(S.read_ply_quads(tmp_path / "closed.ply")[1]) == nfaces


def test_the_other_operators_and_the_element_flag(tmp_path, box_obj):
    import massivevoxelraytracing_amd as mv
    obj, tris = box_obj
    v = tris.reshape(-1, 3)
    lo = v.min(0)
    # (an erosion or an opening of this one-voxel shell would leave nothing, which the library refuses: their methods run in tests/cpp/morph_usage.cpp)
    for op, element, name in (("dilate", mv.MORPH_FACES, "faces"), ("dilate", mv.MORPH_CUBE, "cube"), ("close", mv.MORPH_FACES, "faces")):
        svo = mv.IntersectorOctreeGPU()
        svo.build(v, None, None, None, lo, np.float32((v.max(0) - lo).max() / np.float32(RES)), RES)
        n0 = svo.info().numberOfVoxels
        changed = getattr(svo, op)(element, 1)
        out = subprocess.check_output([APP, obj, str(RES), str(tmp_path / "op.ply"), "--" + op, "1", "--element", name], timeout=120).decode()
        print(out)
        assert "%s: voxels %d -> %d, element %s, steps 1, %s %d" % (op, n0, svo.info().numberOfVoxels, name, "added", changed) in out
    for flags in (["--close", "1", "--open", "1"], ["--close", "0"], ["--close", "1", "--element", "ball"]):
        r = subprocess.run([APP, obj, str(RES), str(tmp_path / "no.ply")] + flags, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--dilate / --erode / --close / --open" in r.stderr and not os.path.exists(tmp_path / "no.ply")


def test_cpp_mirror_runs(tmp_path):
    exe, _ = common.compile_usage(tmp_path, "morph_usage")
    out = subprocess.check_output([str(exe), "run"], timeout=120).decode()
    print(out)
    assert "shell 217 leaky 0 cells 485 peeled 217 plugged 1 enclosed 125 grown 392 opened 0 eroded 348 left 262" in out
