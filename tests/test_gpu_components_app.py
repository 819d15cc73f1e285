"""apps/voxel_mesh --components / --keep-largest / --min-component on meshes written here as OBJ: two solid blocks joined by a bridge one voxel thick, which an
opening cuts (--open 1 --keep-largest 1 leaves one component), and a closed box with debris off its corners (--min-component 2 --fill).  The printed counts equal
those of the Python calls on the same build and of the model.  And the C++ mirror's component methods, compiled and run (tests/cpp/components_usage.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import common
import components_expected as K
from voxel_mesh_app import APP, corners, quad, run, slab, write_obj

pytestmark = pytest.mark.gpu

RES = 32


def dumbbell():
    """in voxel units of a 32^3 grid: horizontal slabs through the middle of the layers z = 4 .. 11 make a solid 8^3 block, z = 5 .. 9 a solid 5^3 block, and one
    narrow strip joins them"""
    v = corners(0.0, 32.0, 0.4)
    for k in range(4, 12):
        v += slab(4.25, 11.75, 4.25, 11.75, k + 0.5)
    for k in range(5, 10):
        v += slab(18.25, 22.75, 5.25, 9.75, k + 0.5)
    v += slab(11.75, 18.25, 7.25, 7.75, 7.5)
    return np.array(v, np.float32).reshape(-1, 3, 3)


def box_with_debris():
    """the closed unit cube inside the grid [-0.2, 1.2]^3, and a small slab through the centre of each of the corner cells (0, 0, 0) and (15, 15, 15) of the 16^3
    grid: voxels of their own, two cells away from the box"""
    v = corners(-0.2, 1.2, 0.02) + slab(-0.19, -0.12, -0.19, -0.12, -0.15625) + slab(1.12, 1.19, 1.12, 1.19, 1.15625)
    for axis in range(3):
        for side in (0.0, 1.0):
            p = [[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]]
            v += quad(*[tuple(np.insert(np.array(q), axis, side)) for q in p])
    return np.array(v, np.float32).reshape(-1, 3, 3)


@pytest.fixture(scope="module")
def objs(tmp_path_factory):
    from massivevoxelraytracing_amd import build as b
    b.build_apps(verbose=False)
    d = tmp_path_factory.mktemp("components_app")
    return {"bell": (write_obj(d / "bell.obj", dumbbell()), dumbbell()), "box": (write_obj(d / "box.obj", box_with_debris()), box_with_debris())}


def built(mv, tris, res):
    v = tris.reshape(-1, 3)
    lo = v.min(0)
    svo = mv.IntersectorOctreeGPU()
    svo.build(v, None, None, None, lo, np.float32((v.max(0) - lo).max() / np.float32(res)), res)
    return svo


def test_components_flag_against_the_model(tmp_path, objs):
    import massivevoxelraytracing_amd as mv
    obj, tris = objs["bell"]
    svo = built(mv, tris, RES)
    x0, _ = svo.read_voxels()
    n0 = len(x0)
    for element, name in ((K.CUBE, "cube"), (K.FACES, "faces")):
        size = np.sort(K.components(x0, RES, element)["size"])[::-1]
        assert size[0] > 500  # the dumbbell (and whatever the two corner triangles leave)
        out = run(obj, RES, tmp_path / "c.ply", "--components", "--element", name)
        assert "components: %d, element %s, largest %s\n" % (len(size), name, " ".join(str(s) for s in size[:5])) in out
        assert "voxels %d faces" % n0 in out  # nothing changed
    many = run(obj, RES, tmp_path / "c.ply", "--erode", "1", "--components")  # counted behind the operator
    svo.erode(mv.MORPH_CUBE, 1)
    size = np.sort(K.components(svo.read_voxels()[0], RES, K.CUBE)["size"])[::-1]
    assert "components: %d, element cube, largest %s\n" % (len(size), " ".join(str(s) for s in size[:5])) in many and many.index("erode:") < many.index("components:")


def test_open_then_keep_largest_leaves_one_component(tmp_path, objs):
    import massivevoxelraytracing_amd as mv
    obj, tris = objs["bell"]
    svo = built(mv, tris, RES)
    n0 = svo.info().numberOfVoxels
    opened = svo.open(mv.MORPH_CUBE, 1)
    x1, a1 = svo.read_voxels()
    before = K.components(x1, RES, K.CUBE)["size"]
    assert sorted(before.tolist()) == [125, 512]  # the bridge and the specks are gone, the blocks stand apart
    removed, kept = svo.keep_components(mv.MORPH_CUBE, keep_largest=1)
    assert (removed, kept) == (125, 1) and len(K.components(svo.read_voxels()[0], RES, K.CUBE)["size"]) == 1
    out = run(obj, RES, tmp_path / "one.ply", "--open", "1", "--keep-largest", "1", "--components")
    assert "open: voxels %d -> %d, element cube, steps 1, removed %d" % (n0, len(x1), opened) in out
    assert "components: 2, element cube, largest 512 125\n" in out
    assert "keep: voxels %d -> 512, components 2 -> 1, element cube, removed 125" % len(x1) in out
    assert out.index("open:") < out.index("components:") < out.index("keep:") and "voxels 512 faces %d " % svo.surface_masks()[1] in out
    for flags in (["--keep-largest", "0"], ["--min-component", "0"], ["--keep-largest", "-3", "--min-component", "2"]):
        r = subprocess.run([APP, obj, str(RES), str(tmp_path / "no.ply")] + flags, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--keep-largest" in r.stderr and not os.path.exists(tmp_path / "no.ply")


def test_min_component_then_fill(tmp_path, objs):
    import massivevoxelraytracing_amd as mv
    obj, tris = objs["box"]
    svo = built(mv, tris, 16)
    x0, a0 = svo.read_voxels()
    sizes = K.components(x0, 16, K.CUBE)["size"]
    assert sorted(sizes.tolist())[:2] == [1, 1] and len(sizes) == 3
    removed, kept = svo.keep_components(mv.MORPH_CUBE, min_voxels=2)
    assert (removed, kept) == (2, 1) and np.array_equal(svo.read_voxels()[0], K.keep(x0, a0, 16, K.CUBE, 2)[0])
    n1 = svo.info().numberOfVoxels
    cells, regions = svo.enclosed_cells_device()
    assert cells > 100 and regions == 1 and svo.fill_enclosed() == cells
    out = run(obj, 16, tmp_path / "box.ply", "--min-component", "2", "--fill")
    assert "keep: voxels %d -> %d, components 3 -> 1, element cube, removed 2" % (len(x0), n1) in out
    assert "fill: voxels %d -> %d, enclosed cells %d in 1 regions, filled %d" % (n1, n1 + cells, cells, cells) in out
    assert out.index("keep:") < out.index("fill:") and "voxels %d faces %d " % (n1 + cells, svo.surface_masks()[1]) in out


def test_cpp_mirror_runs(tmp_path):
    exe, _ = common.compile_usage(tmp_path, "components_usage")
    out = subprocess.check_output([str(exe), "run"], timeout=120).decode()
    print(out)
    assert "voxels 221 faces 4 largest 218 cube 3 listed 1 specks 1 kept 2 debris 2 none 0 left 218" in out
