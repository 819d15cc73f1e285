"""apps/voxel_mesh --lod and apps/rtcamp_batch --lod on the bunny: the mesh is that of the coarsened voxel set, with the model's voxel count in the report line and
the faces of surface_masks of the coarsened octree in the PLY; the batch driver reports the same coarsening and writes its frame."""
import os
import re
import subprocess

import numpy as np
import pytest

import coarsen_expected as X
import surface_expected as S
from common import GOLDEN, bunny_tris
from voxel_mesh_app import write_reader_obj

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("extra,min_count", [([], 1), (["--lod-min-count", "3"], 3), (["--no-weld", "--fill"], 1)])
def test_voxel_mesh_lod(tmp_path, extra, min_count):
    import massivevoxelraytracing_amd as mv
    from massivevoxelraytracing_amd import build as b
    b.build_apps(verbose=False)
    tris = bunny_tris()
    write_reader_obj(tmp_path / "bunny.obj", tris)
    out = subprocess.check_output([os.path.join(ROOT, "apps", "voxel_mesh"), str(tmp_path / "bunny.obj"), "64", str(tmp_path / "bunny.ply"), "--lod", "1"] + extra, timeout=120).decode()
    print(out)
    v = tris.reshape(-1, 3)
    lo = v.min(0)
    dps = np.float32((v.max(0) - lo).max() / np.float32(64))
    svo = mv.IntersectorOctreeGPU()
    svo.build(v, None, None, None, lo, dps, 64)
    xyz, attribs = svo.read_voxels()
    want = X.coarse(xyz, attribs, 1, min_count)
    assert len(xyz) == 8516 and "lod: voxels 8516 -> %d, gridRes 64 -> 32" % len(want["xyz"]) in out
    svo.coarsen(1, min_count)
    if "--fill" in extra:
        assert svo.fill_enclosed() > 0
    masks, n_faces = svo.surface_masks()
    vertices, indices, colours = S.read_ply_quads(tmp_path / "bunny.ply")
    assert len(indices) == n_faces and "voxels %d faces %d vertices %d" % (svo.info().numberOfVoxels, n_faces, len(vertices)) in out
    if not extra:  # the mesh of the model's list at the coarse grid, vertex for vertex
        mesh = S.surface(want["xyz"], 32, lo, np.float32(dps * np.float32(2)))
        assert mesh["nFaces"] == n_faces and np.array_equal(np.ascontiguousarray(vertices).view(np.uint32), mesh["vertices"].view(np.uint32))
        assert np.array_equal(indices, mesh["indices"]) and np.array_equal(colours, want["attribs"][mesh["faceVoxel"], :3])


def test_batch_driver_lod(tmp_path):
    from massivevoxelraytracing_amd import build as b
    exe = b.build_apps(verbose=False)
    obj = tmp_path / "bunny.obj"
    write_reader_obj(obj, bunny_tris())
    out = tmp_path / "out"
    os.mkdir(out)
    W, H = 96, 54
    text = subprocess.check_output([exe, str(obj), os.path.join(GOLDEN, "monks_forest_s.hdr"), str(out), "--frames", "8", "--frame-range", "5", "6", "--size", str(W), str(H),
                                    "--res", "64", "256", "--steps", "2", "--lod", "1"], timeout=120).decode()
    print(text)
    m = re.search(r"lod: voxels (\d+) -> (\d+), gridRes (\d+) -> (\d+)", text)
    assert m, text
    fine, coarse, res, coarse_res = (int(x) for x in m.groups())
    assert coarse_res * 2 == res and fine / 6 < coarse < fine / 2  # a surface: about a quarter of the voxels one level up
    ppm = open(out / "005.ppm", "rb").read()
    head = len(b"P6\n%d %d\n255\n" % (W, H))
    assert len(ppm) == head + W * H * 3 and len(np.unique(np.frombuffer(ppm[head:], np.uint8))) > 20
