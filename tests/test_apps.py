"""Host applications on top of the boundary (apps/): file formats on CPU, the RTCamp-style batch driver on the GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import common
from common import GOLDEN, bunny_tris
from voxel_mesh_app import read_png_rgba, write_reader_obj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scene_io_formats(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "io_check"
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "apps"), os.path.join(ROOT, "tests", "cpp", "io_check.cpp"), "-o", str(exe)])
    tris = bunny_tris()[:500]
    obj = tmp_path / "m.obj"
    write_reader_obj(obj, tris, with_colors=True)
    out = subprocess.check_output([str(exe), str(obj), str(tmp_path / "a.png"), str(tmp_path / "a.ppm")]).split()
    v = np.loadtxt(obj, comments=["#", "f"], usecols=(1, 2, 3, 4, 5, 6), dtype=np.float64, converters={0: lambda s: 0.0}) if False else None
    pts = tris.reshape(-1, 3).astype(np.float64)
    assert int(out[0]) == len(pts)
    assert abs(float(out[1]) - (pts[:, 0] + 2 * pts[:, 1] + 3 * pts[:, 2]).sum()) < 1e-3
    lo = pts.min(0)
    assert np.allclose([float(x) for x in out[3:6]], lo, atol=1e-6)
    assert abs(float(out[6]) - (pts.max(0) - lo).max() / 256) < 1e-7
    img = read_png_rgba(tmp_path / "a.png")
    H, W = 23, 37
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    want = np.stack([(x * 7) & 255, (y * 11) & 255, x ^ y, np.full_like(x, 255)], -1).astype(np.uint8)
    assert np.array_equal(img, want)
    ppm = open(tmp_path / "a.ppm", "rb").read()
    assert ppm.startswith(b"P6\n37 23\n255\n") and np.array_equal(np.frombuffer(ppm[len(b"P6\n37 23\n255\n"):], np.uint8).reshape(H, W, 3), want[..., :3])


def test_batch_driver_builds():
    from massivevoxelraytracing_amd import build as b
    exe = b.build_apps(verbose=False)
    out = subprocess.check_output([exe])
    assert b"--frame-range" in out


@pytest.mark.gpu
def test_batch_driver_frames_match_the_oracle(tmp_path):
    """3 frames of the C++ driver (apps/rtcamp_batch: per-frame rebuild with the resolution ramp, N steps per frame, async writer,
    frame-range sharding -- RTCamp.cpp:111-193 / run.py:11-27 semantics) == the ORACLE rendering the same frames: the oracle voxelizes the
    triangles at the driver's per-frame grid, path-traces `steps` iterations with the driver's own camera matrices and resolves to bytes."""
    from massivevoxelraytracing_amd import build as b
    from oracle import oracle as O
    exe = b.build_apps(verbose=False)
    tris = bunny_tris()
    obj = tmp_path / "bunny.obj"
    write_reader_obj(obj, tris)
    hdr = os.path.join(GOLDEN, "monks_forest_s.hdr")
    W, H, steps = 160, 90, 3
    subprocess.check_call([exe, str(obj), hdr, str(tmp_path), "--frames", "8", "--frame-range", "4", "7", "--size", str(W), str(H), "--res", "64", "1024", "--steps", str(steps),
                           "--dump-cameras"])
    v = tris.reshape(-1, 3)
    emis = np.zeros_like(v)
    lo = v.min(0)
    ext = np.float32((v.max(0) - lo).max())
    emis[v[:, 1] > lo[1] + np.float32(0.94) * ext] = np.array([1.0, 0.85, 0.6], np.float32)
    rgba, hw, hh = O.decode_rgbe(open(hdr, "rb").read())
    Hd = O.HDRI(rgba, hw, hh, rgba, hw, hh, math_mode=1)
    grids = set()
    for frame in (4, 5, 6):
        lines = open(tmp_path / ("%03d.camera.txt" % frame)).read().split("\n")
        view = np.array([float.fromhex(t) for t in lines[0].split()], np.float32)
        proj = np.array([float.fromhex(t) for t in lines[1].split()], np.float32)
        t = lines[2].split()
        focus, lens_r, ox, oy, oz, dps = (float.fromhex(x) for x in t[:6])
        grid = int(t[6])
        grids.add(grid)
        sc = O.build_scene_from_triangles(tris, grid, np.ones_like(v).reshape(-1, 9), emis.reshape(-1, 9), origin=np.array([ox, oy, oz], np.float32), dps=np.float32(dps))
        cam = O.camera_from_matrices(view, proj, focus, lens_r)
        fb = np.zeros((W * H, 4), np.float32)
        for it in range(steps):
            fb, _, _ = sc.render_pt(Hd, cam, W, H, it, math_mode=1, fb=fb, threads=8)
        want = O.resolve(fb, math_mode=1)
        ppm = open(tmp_path / ("%03d.ppm" % frame), "rb").read()
        hdr_len = len(b"P6\n%d %d\n255\n" % (W, H))
        got = np.frombuffer(ppm[hdr_len:], np.uint8).reshape(H * W, 3)
        assert np.array_equal(got, want[:, :3]), frame
        assert got.max() > 0
    assert len(grids) >= 2  # the resolution ramp really changed the grid between frames
    assert not os.path.exists(tmp_path / "003.ppm") and not os.path.exists(tmp_path / "007.ppm")  # frame-range sharding


@pytest.mark.gpu
def test_tile_render_single_process_rccl_matches_the_oracle(tmp_path):
    """apps/tile_render: the native multi-GPU host path (one process, one PathTracer + one RCCL communicator per device, tile split,
    ncclAllGather of the accumulation buffers, assemble, resolve).  Run on the GPUs this box has (1): the collective and the assembly
    really execute, and the gathered frame equals the ORACLE's frame bit for bit -- float accumulation buffer and resolved bytes."""
    from massivevoxelraytracing_amd import build as b
    from oracle import oracle as O
    b.build_apps(verbose=False)
    exe = os.path.join(ROOT, "apps", "tile_render")
    tris = bunny_tris()
    obj = tmp_path / "bunny.obj"
    write_reader_obj(obj, tris)
    hdr = os.path.join(GOLDEN, "monks_forest_s.hdr")
    W, H, steps, res = 200, 113, 2, 128
    out = subprocess.check_output([exe, str(obj), hdr, str(tmp_path / "f.ppm"), "--gpus", "8", "--size", str(W), str(H), "--res", str(res), "--steps", str(steps),
                                   "--dump-f32", str(tmp_path / "f.f32"), "--dump-camera", str(tmp_path / "cam.txt")]).decode()
    assert "devices" in out and "best frame" in out
    lines = open(tmp_path / "cam.txt").read().split("\n")
    view = np.array([float.fromhex(t) for t in lines[0].split()], np.float32)
    proj = np.array([float.fromhex(t) for t in lines[1].split()], np.float32)
    t = lines[2].split()
    focus, lens_r, ox, oy, oz, dps = (float.fromhex(x) for x in t[:6])
    assert int(t[6]) == res
    v = tris.reshape(-1, 3)
    emis = np.zeros_like(v)
    lo = v.min(0)
    ext = np.float32((v.max(0) - lo).max())
    emis[v[:, 1] > lo[1] + np.float32(0.94) * ext] = np.array([1.0, 0.85, 0.6], np.float32)
    sc = O.build_scene_from_triangles(tris, res, np.ones_like(v).reshape(-1, 9), emis.reshape(-1, 9), origin=np.array([ox, oy, oz], np.float32), dps=np.float32(dps))
    rgba, hw, hh = O.decode_rgbe(open(hdr, "rb").read())
    Hd = O.HDRI(rgba, hw, hh, rgba, hw, hh, math_mode=1)
    cam = O.camera_from_matrices(view, proj, focus, lens_r)
    fb = np.zeros((W * H, 4), np.float32)
    for it in range(steps):
        fb, _, _ = sc.render_pt(Hd, cam, W, H, it, math_mode=1, fb=fb, threads=8)
    got = np.fromfile(tmp_path / "f.f32", np.float32).reshape(W * H, 4)
    assert np.array_equal(got, fb)
    ppm = open(tmp_path / "f.ppm", "rb").read()
    hdr_len = len(b"P6\n%d %d\n255\n" % (W, H))
    assert np.array_equal(np.frombuffer(ppm[hdr_len:], np.uint8).reshape(H * W, 3), O.resolve(fb, math_mode=1)[:, :3])


@pytest.mark.gpu
def test_bench_rccl_branch_runs_on_one_gpu():
    """bench.py's N > 1 code path (torch.distributed over RCCL: d2d copy of the accumulation buffer, all_gather_into_tensor, assemble on
    the device, all ordered on one stream) executed with a world of ONE rank (MVRT_FORCE_DIST=1), in a fresh process; the line reports
    that every rank found its own pixels, bit for bit, in the assembled frame."""
    import json
    import socket
    import sys
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, MVRT_FORCE_DIST="1", RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1", "--width", "640", "--height", "360", "--grid-res", "512",
                                   "--detail", "0.25", "--no-cpu-baseline", "--full"], env=env, timeout=600).decode()
    line = json.loads(out.strip().split("\n")[-1])
    assert line["n_gpus"] == 1 and line["value"] > 0 and line["config"]["gather_ok"] is True
    assert "RCCL" in line["config"]["parallelism"]


@pytest.mark.gpu
def test_bench_self_launches_its_ranks():
    """`python bench.py --gpus N` with NO launcher and no WORLD_SIZE: bench.py starts torch.distributed.run itself (a child process, before it touches
    the GPU) and relays rank 0's line.  Driven here with N = 1 + MVRT_FORCE_DIST=1 (a box has one GPU): the RCCL gather path runs and every
    rank finds its pixels in the assembled frame."""
    import json
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(MVRT_FORCE_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1", "--width", "640", "--height", "360", "--grid-res", "512",
                                   "--detail", "0.25", "--no-cpu-baseline", "--full"], env=env, timeout=900).decode()
    line = json.loads(out.strip().split("\n")[-1])
    assert line["n_gpus"] == 1 and line["n_ranks_seen"] == 1 and line["value"] > 0 and line["config"]["gather_ok"] is True
    assert "RCCL" in line["config"]["parallelism"]


@pytest.mark.gpu
def test_cpp_mirror_frame_buffer_members(tmp_path):
    """the reference's public members a caller reads (PathTracer.hpp:23-27): RTCamp.cpp:169 copies pt.m_frameBufferU8->data() device to device
    after resolve(); m_steps counts step() calls.  tests/cpp/mirror_usage.cpp does exactly that on the header-only mirror."""
    import shutil as sh
    import massivevoxelraytracing_amd as mv
    exe, libdir = common.compile_usage(tmp_path, "mirror_usage")
    sh.copy(os.path.join(GOLDEN, "monks_forest_s.hdr"), tmp_path / "monks_forest_s.hdr")
    out = subprocess.check_output([str(exe), "run"], cwd=tmp_path, timeout=300).decode()
    assert "steps 1 " in out
    assert "m_steps 1 u8 bytes %d f32 bytes %d same 1 sumW %.1f" % (64 * 36 * 4, 64 * 36 * 16, 64 * 36 * 16.0) in out
