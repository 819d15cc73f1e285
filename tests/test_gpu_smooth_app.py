"""The layers above mvrt_svo_surface_smooth on a GPU: apps/voxel_mesh --smooth on the bunny at 64^3, whose PLY must hold the vertices and indices of the numpy
model (tests/smooth_expected.py) on the voxel set the build made and whose line of counts must name them, alone and with --exterior; the refusal together with
--merge and --no-weld; and tests/cpp/smooth_usage.cpp through the C++ mirror."""
import os
import subprocess

import numpy as np
import pytest

import common
import smooth_expected as M
import surface_expected as S
from common import bunny_tris
from fixtures import mv  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "apps", "voxel_mesh")


@pytest.fixture(scope="module")
def bunny(mv, tmp_path_factory):
    from massivevoxelraytracing_amd import build as b
    b.build_apps(verbose=False)
    tris = bunny_tris()
    v = tris.reshape(-1, 3)
    obj = tmp_path_factory.mktemp("smooth") / "bunny.obj"
    with open(obj, "w") as f:
        f.write("".join("v %.9g %.9g %.9g\n" % tuple(p) for p in v) + "".join("f %d %d %d\n" % (3 * t + 1, 3 * t + 2, 3 * t + 3) for t in range(len(tris))))
    lo = v.min(0)
    dps = np.float32((v.max(0) - lo).max() / np.float32(64))
    svo = mv.IntersectorOctreeGPU()
    svo.build(v, None, None, None, lo, dps, 64)
    return obj, svo, lo, dps


@pytest.mark.parametrize("flags,K,weights,limit", [([], 4, (256, 256), 127), (["--exterior"], 4, (256, 256), 127), (["--smooth-taubin", "--smooth-limit", "100"], 4, (128, -136), 100)])
def test_voxel_mesh_smooth(mv, bunny, tmp_path, flags, K, weights, limit):
    obj, svo, lo, dps = bunny
    ply = tmp_path / "bunny.ply"
    out = subprocess.check_output([APP, str(obj), "64", str(ply), "--smooth", str(K)] + flags, timeout=120).decode()
    xyz, attrs = svo.read_voxels()
    masks = svo.surface_exterior_masks()[0] if "--exterior" in flags else None
    want = M.smooth(xyz, 64, lo, dps, K, weights, limit, masks)
    vertices, indices, colours = S.read_ply_quads(ply)
    assert np.array_equal(vertices.view(np.uint32), want["vertices"].view(np.uint32)) and np.array_equal(indices, want["indices"])
    assert np.array_equal(colours, attrs[want["faceVoxel"], :3])
    assert "faces %d vertices %d smooth %d weights %d %d limit %d clamped %d " % (len(indices), len(vertices), K, weights[0], weights[1], limit, want["clamped"]) in out
    assert want["displacements"].any()


@pytest.mark.parametrize("other", ["--merge", "--merge-any", "--no-weld"])
def test_voxel_mesh_refuses_smooth_with_merge_and_no_weld(bunny, tmp_path, other):
    obj = bunny[0]
    done = subprocess.run([APP, str(obj), "64", str(tmp_path / "no.ply"), "--smooth", "4", other], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert done.returncode != 0 and "--smooth cannot be combined" in done.stderr and not (tmp_path / "no.ply").exists()


def test_cpp_mirror_runs(tmp_path, mv):
    exe, libdir = common.compile_usage(tmp_path, "smooth_usage")
    out = subprocess.check_output([str(exe), "run"], timeout=120).decode()
    assert "faces 24 vertices 26 clamped 120 moved 26 none 0 same 1 top faces 8 vertices 18 clamped 88 sizing 0" in out
