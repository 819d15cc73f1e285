"""Adaptive sampling without a GPU: the helper of the GPU tests (tests/adaptive_expected.py) is pinned to the oracle's own path tracer, the error-mask recipe is
checked on hand-made rows, one per rule of include/mvrt.h, every host-side refusal of mvrt_pt_set_sample_mask / mvrt_pt_error_mask is exercised, and the entry
points exist in every layer."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import common
import adaptive_expected as X
from common import bunny_tris, hdr_bytes, position_colors, probe_camera

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NAMES = ["mvrt_pt_set_sample_mask", "mvrt_pt_active_pixels", "mvrt_pt_error_mask"]


def _err(lib):
    return lib.mvrt_last_error().decode()


def test_all_ones_mask_reproduces_the_oracle_frame_buffer():
    """two iterations, 32 x 18, bunny 256^3: the helper with every pixel active == render_pt's own fb, and a pixel that sits out keeps its bits"""
    from oracle import oracle as O
    tris = bunny_tris()
    cols, emis = position_colors(tris)
    sc = O.build_scene_from_triangles(tris, 256, cols, emis)
    rgba, hw, hh = O.decode_rgbe(hdr_bytes())
    Hd = O.HDRI(rgba, hw, hh, rgba, hw, hh, math_mode=1)
    w, h = 32, 18
    cam = probe_camera(sc.origin, sc.dps, 256, focus=9.0, lens_r=0.05)
    exp = X.Expected(O, sc, Hd, w, h, aovs=False)
    fb = np.zeros((w * h, 4), f32)
    for it in range(2):
        exp.step(cam, np.ones(w * h, np.uint8))
        fb, sl, _ = sc.render_pt(Hd, cam, w, h, it, math_mode=1, fb=fb, want_samples=True, threads=8)
        assert np.array_equal(exp.samples, sl)
    assert np.array_equal(exp.fb.view(np.uint32), fb.view(np.uint32)) and (fb[:, 3] == 32).all() and fb[:, 0:3].any()
    # a third iteration on every other pixel: those get iteration 2's samples, the rest nothing
    mask = (np.arange(w * h) % 2 == 0)
    before = exp.fb.copy()
    exp.step(cam, mask)
    fb3, sl3, _ = sc.render_pt(Hd, cam, w, h, 2, math_mode=1, fb=fb.copy(), want_samples=True, threads=8)
    assert np.array_equal(exp.fb[mask], fb3[mask]) and np.array_equal(exp.fb[~mask], before[~mask]) and exp.steps == 3
    assert np.array_equal(exp.samples, sl3.reshape(-1, 16, 3)[mask].reshape(-1, 3))  # the compact numbering


def test_error_mask_recipe_on_hand_made_rows():
    """one row per rule.  threshold 0.5, floor 0.25, min 32, max 64"""
    def row(n, s1, s2):
        return [0, 0, 0, n], [s1, s2, 0, 0]
    rows = [
        row(0, 0, 0),          # n = 0: active
        row(16, 16, 16),       # n < min (zero variance all the same): active
        row(64, 64, 6400),     # n >= max, however noisy: inactive
        row(32, 32, 32),       # zero variance (m2 == m1 * m1): inactive
        row(32, 1, 4),         # m1 = 1/32 below the floor: var = (1/8 - 1/1024) / 31, se ~ 0.0632 > 0.5 * 0.25 is false: inactive
        row(32, 1, 64),        # same mean, se = sqrt( (2 - 1/1024) / 31 ) ~ 0.254 > 0.125: active -- against the mean (0.0156) the row above were active too
        row(32, 64, 1120),     # se EXACTLY the bound: m1 = 2, m2 = 35, var = ( 35 - 4 ) / 31 = 1, se = 1 = 0.5 * 2 (every step exact in fp32): inactive
    ]
    fb = np.array([r[0] for r in rows], f32)
    mo = np.array([r[1] for r in rows], f32)
    got = X.error_mask(fb, mo, 0.5, lum_floor=0.25, min_samples=32, max_samples=64)
    assert got.dtype == np.uint8 and got.tolist() == [1, 1, 0, 0, 0, 1, 0]
    # the tie is a tie: a little more of s2 tips it (var = 1.001, se = 1.0005)
    mo2 = mo.copy()
    mo2[-1, 1] = 1121
    assert X.error_mask(fb, mo2, 0.5, 0.25, 32, 64)[-1] == 1
    # the floor row: against its own mean it would be active
    assert X.error_mask(fb[4:5], mo[4:5], 0.5, lum_floor=1e-3, min_samples=32, max_samples=64)[0] == 1
    # no maximum: the noisy n = 64 row is active
    assert X.error_mask(fb[2:3], mo[2:3], 0.5, 0.25, 32, 0)[0] == 1


def test_host_side_refusals_without_a_gpu():
    """null handle, no frame, bad threshold / floor / min / max, null mask array, moments off: refused before any GPU call, with a message that names the reason"""
    import massivevoxelraytracing_amd as mv
    lib = mv.lib()
    fake = 0x1000  # never dereferenced
    n = C.c_uint64(7)
    assert lib.mvrt_pt_set_sample_mask(None, None, fake, C.byref(n)) != 0 and "null" in _err(lib)
    assert lib.mvrt_pt_error_mask(None, None, 0.1, 0.01, 32, 0, fake, C.byref(n)) != 0 and "null" in _err(lib)
    assert lib.mvrt_pt_active_pixels(None) == 0
    h = C.c_void_p(0)
    assert lib.mvrt_pt_create(C.byref(h)) == 0
    try:
        assert lib.mvrt_pt_active_pixels(h) == 0
        for mask in (fake, None):
            assert lib.mvrt_pt_set_sample_mask(h, None, mask, C.byref(n)) != 0 and "no frame buffer" in _err(lib)
        assert lib.mvrt_pt_error_mask(h, None, 0.1, 0.01, 32, 0, fake, C.byref(n)) != 0 and "mvrt_pt_set_moments" in _err(lib)
        assert lib.mvrt_pt_set_moments(h, 1) == 0
        assert lib.mvrt_pt_error_mask(h, None, 0.1, 0.01, 32, 0, fake, C.byref(n)) != 0 and "no frame buffer" in _err(lib)
        assert lib.mvrt_pt_error_mask(h, None, 0.1, 0.01, 32, 0, None, C.byref(n)) != 0 and "null" in _err(lib)
        for args, word in (((0.0, 0.01, 32, 0), "threshold"), ((-1.0, 0.01, 32, 0), "threshold"), ((float("nan"), 0.01, 32, 0), "threshold"), ((0.1, 0.0, 32, 0), "lumFloor"),
                           ((0.1, float("nan"), 32, 0), "lumFloor"), ((0.1, 0.01, 0, 0), "minSamples"), ((0.1, 0.01, 32, -1), "maxSamples")):
            assert lib.mvrt_pt_error_mask(h, None, *args, fake, C.byref(n)) != 0 and word in _err(lib), args
        assert n.value == 7  # a refused call writes nothing
    finally:
        lib.mvrt_pt_destroy(h)
    # the Python mirror raises on them
    pt = mv.PathTracer()
    with pytest.raises(mv.MvrtError, match="no frame buffer"):
        pt.set_sample_mask(None)
    with pytest.raises(mv.MvrtError, match="mvrt_pt_set_moments"):
        pt.error_mask(0.1)
    assert pt.active_pixels() == 0
    pt.cleanUp()


def test_entry_points_exist_in_every_layer(tmp_path):
    """header (each new entry marked "new; the reference has none"), library, Python mirror, C++ mirror (tests/cpp/adaptive_usage.cpp compiles with -Werror and
    its GPU-free part runs)"""
    import massivevoxelraytracing_amd as mv
    text = open(os.path.join(ROOT, "include", "mvrt.h")).read()
    lib = C.CDLL(mv.LIB_PATH)
    for s in NAMES:
        m = re.search(r"^[a-z][^\n]*\b%s\s*\([^\n]*$" % s, text, re.M)  # the declaration's line
        assert m, s
        before = text[: m.start()].rstrip()
        comment = before[before.rindex("/*"):] if before.endswith("*/") else ""
        assert "new; the reference has none" in comment + m.group(0), s
        assert hasattr(lib, s) and s in mv.SIGNATURES, s
    assert "se > threshold * max( m1, lumFloor )" in text  # the formula is written out in the header
    for m in ("set_sample_mask", "active_pixels", "error_mask"):
        assert callable(getattr(mv.PathTracer, m))
    exe, libdir = common.compile_usage(tmp_path, "adaptive_usage", missing="fail")
    out = subprocess.check_output([str(exe)], env=dict(os.environ, LD_LIBRARY_PATH=libdir + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", "")))
    assert b"refused 1 1 active 0" in out
