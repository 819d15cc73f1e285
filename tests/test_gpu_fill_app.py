"""apps/voxel_mesh --fill: the bunny at 64^3 with its enclosed cells filled before the surface is extracted.  The PLY holds the faces of the filled set, the
model's count, and the report line names the voxels before and after and the cell and region counts."""
import os
import subprocess

import numpy as np
import pytest

import fill_expected as F
import surface_expected as S
from common import bunny_tris

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("extra", [[], ["--no-weld"], ["--merge"], ["--ao", "16"]])
def test_voxel_mesh_fill(tmp_path, extra):
    import massivevoxelraytracing_amd as mv
    from massivevoxelraytracing_amd import build as b
    b.build_apps(verbose=False)
    tris = bunny_tris()
    v = tris.reshape(-1, 3)
    with open(tmp_path / "bunny.obj", "w") as f:
        f.write("".join("v %.9g %.9g %.9g\n" % tuple(p) for p in v) + "".join("f %d %d %d\n" % (3 * t + 1, 3 * t + 2, 3 * t + 3) for t in range(len(tris))))
    out = subprocess.check_output([os.path.join(ROOT, "apps", "voxel_mesh"), str(tmp_path / "bunny.obj"), "64", str(tmp_path / "bunny.ply"), "--fill"] + extra, timeout=120).decode()
    print(out)
    lo = v.min(0)
    dps = np.float32((v.max(0) - lo).max() / np.float32(64))
    svo = mv.IntersectorOctreeGPU()
    svo.build(v, None, None, None, lo, dps, 64)
    xyz, _ = svo.read_voxels()
    cells = F.enclosed(xyz, 64)
    want = S.surface(F.filled_set(xyz, 64), 64, lo, dps)
    n, c, r = len(xyz), len(cells["xyz"]), cells["nRegions"]
    assert "fill: voxels %d -> %d, enclosed cells %d in %d regions, filled %d" % (n, n + c, c, r, c) in out
    assert (n, c, r, want["nFaces"]) == (8516, 48162, 3, 14558)  # the oracle's numbers (tests/test_fill_cpu.py)
    vertices, indices, colours = S.read_ply_quads(tmp_path / "bunny.ply")
    if extra == ["--merge"]:
        assert "faces %d rects %d" % (want["nFaces"], len(indices)) in out and len(indices) < want["nFaces"]
        return
    assert len(indices) == want["nFaces"] and "faces %d vertices %d" % (len(indices), len(vertices)) in out
    if extra != ["--no-weld"]:
        assert np.array_equal(np.ascontiguousarray(vertices).view(np.uint32), want["vertices"].view(np.uint32)) and np.array_equal(indices, want["indices"])
    # every face belongs to a voxel of the shell: a fill voxel has voxels and fill voxels for neighbours, never an empty cell
    assert svo.fill_enclosed() == c
    if extra == ["--ao", "16"]:  # the colours are scaled by the open fraction: the bake ran on the filled octree's own face list (the app checks that itself)
        return
    _, attrs = svo.read_voxels()
    assert np.array_equal(colours, attrs[want["faceVoxel"], :3]) and np.isin(S.morton(S.sorted_voxels(F.filled_set(xyz, 64))[want["faceVoxel"]]), S.morton(xyz)).all()
