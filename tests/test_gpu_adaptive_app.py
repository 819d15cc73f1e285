"""apps/rtcamp_batch --adaptive on the bunny at a small size: the frame is written, the samples it reports are fewer than steps * pixels * 16, and the frame
replayed through the Python binding with the same loop (error_mask, set_sample_mask every K steps) is the driver's frame, spends the driver's samples and has at
least minSamples samples in every pixel."""
import os
import re
import subprocess

import numpy as np
import pytest

from common import GOLDEN, bunny_tris
from voxel_mesh_app import write_reader_obj

pytestmark = pytest.mark.gpu


def test_batch_driver_adaptive(tmp_path):
    import massivevoxelraytracing_amd as mv
    from massivevoxelraytracing_amd import build as b
    exe = b.build_apps(verbose=False)
    tris = bunny_tris()
    obj = tmp_path / "bunny.obj"
    write_reader_obj(obj, tris)
    hdr_file = os.path.join(GOLDEN, "monks_forest_s.hdr")
    W, H, steps, threshold, every = 96, 54, 8, 0.1, 2
    out = tmp_path / "out"
    os.mkdir(out)
    text = subprocess.check_output([exe, str(obj), hdr_file, str(out), "--frames", "8", "--frame-range", "5", "6", "--size", str(W), str(H), "--res", "64", "256", "--steps", str(steps),
                                    "--dump-cameras", "--adaptive", str(threshold), "--adaptive-every", str(every)]).decode()
    print(text)
    m = re.search(r"\[frame 5\] adaptive: (\d+) of (\d+) steps, (\d+) of (\d+) samples", text)
    assert m, text
    taken, of_steps, spent, full = (int(x) for x in m.groups())
    assert of_steps == steps and full == steps * W * H * 16
    assert 2 <= taken <= steps and 2 * W * H * 16 <= spent < full
    ppm = open(out / "005.ppm", "rb").read()
    head = len(b"P6\n%d %d\n255\n" % (W, H))
    assert len(ppm) == head + W * H * 3
    frame = np.frombuffer(ppm[head:], np.uint8).reshape(H * W, 3)
    assert len(np.unique(frame)) > 20
    # the same frame through the Python binding
    lines = open(out / "005.camera.txt").read().split("\n")
    view = np.array([float.fromhex(t) for t in lines[0].split()], np.float32)
    proj = np.array([float.fromhex(t) for t in lines[1].split()], np.float32)
    t = lines[2].split()
    focus, lens_r, ox, oy, oz, dps = (float.fromhex(x) for x in t[:6])
    res = int(t[6])
    v = tris.reshape(-1, 3)
    pt = mv.PathTracer()
    pt.setup(None)
    pt.set_moments(True)
    pt.resizeFrameBufferIfNeeded(None, W, H)
    pt.loadHDRI(None, hdr_file, hdr_file)
    lo = v.min(0)
    wide = float((v.max(0) - lo).max())
    emis = np.zeros_like(v)
    emis[v[:, 1] > lo[1] + np.float32(0.94) * np.float32(wide)] = [1.0, 0.85, 0.6]
    pt.updateScene(v, np.ones_like(v), emis, None, np.array([ox, oy, oz], np.float32), np.float32(dps), res)
    mask_dev = mv.DeviceArray(pt.owned_pixels(), np.uint8)
    my_taken = my_spent = 0
    for it in range(steps):
        if it >= 2 and (it - 2) % every == 0:
            pt.error_mask(threshold, 0.01, 32, 0, out_dev=mask_dev)
            if pt.set_sample_mask(mask_dev) == 0:
                break
        pt.step(None, (view, proj), focus, lens_r)
        my_taken += 1
        my_spent += pt.active_pixels() * 16
    assert (my_taken, my_spent) == (taken, spent)
    fb = pt.read_framebuffer()[: W * H]
    assert (fb[:, 3] >= 32).all() and fb[:, 3].sum() == spent and fb[:, 3].min() < fb[:, 3].max()
    assert np.array_equal(frame, pt.toImageAsync()[: W * H, 0:3]), "the replay renders the driver's frame"
