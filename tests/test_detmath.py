"""include/mvrt_detmath.h against libm, and what swapping libm for it does to an image."""
import numpy as np

from common import bunny_tris, hdr_bytes, position_colors, probe_camera
from oracle import oracle as O


def ulp_err(got, want):
    want32 = want.astype(np.float32)
    ulp = np.spacing(np.abs(want32)).astype(np.float64)
    return np.abs(got.astype(np.float64) - want) / ulp


def test_sin_cos_accuracy():
    x = np.linspace(-4 * np.pi, 4 * np.pi, 2_000_001).astype(np.float32)
    # absolute error: near zeros of sin/cos the Cody-Waite remainder limits relative accuracy
    assert np.abs(O.detmath("sin", x).astype(np.float64) - np.sin(x.astype(np.float64))).max() < 2.5e-7
    assert np.abs(O.detmath("cos", x).astype(np.float64) - np.cos(x.astype(np.float64))).max() < 2.5e-7


def test_atan2_accuracy():
    rng = np.random.default_rng(0)
    y = rng.normal(size=1_000_000).astype(np.float32)
    x = rng.normal(size=1_000_000).astype(np.float32)
    got = O.detmath("atan2", x, y)
    assert np.abs(got.astype(np.float64) - np.arctan2(y.astype(np.float64), x.astype(np.float64))).max() < 1e-6
    assert O.detmath("atan2", np.zeros(1, np.float32), np.zeros(1, np.float32))[0] == 0.0


def test_pow_gamma_accuracy():
    x = np.exp(np.linspace(np.log(1e-6), np.log(64.0), 1_000_001)).astype(np.float32)
    y = np.full_like(x, np.float32(1.0 / 2.2))
    got = O.detmath("pow", x, y)
    want = np.power(x.astype(np.float64), np.float64(np.float32(1.0 / 2.2)))
    assert (np.abs(got - want) / want).max() < 2e-6
    assert O.detmath("pow", np.zeros(1, np.float32), y[:1])[0] == 0.0


def test_resolve_outside_the_ordinary_range():
    """the oracle's resolve on the rows of tests/denoise_cases.py: NaN, negative means and 0 / 0 give 0, every mean whose scaled value is at least 255 gives 255
    (include/mvrt.h, mvrt_resolve_buffer).  With the conversion to int taken before the clamp, x86 turned 1e16, 1e20, 3e38, +inf and x / 0 into 0: the second, fourth and
    fifth row came out as (0,0,0), (0,255,0) and (0,0,0).  The ordinary range around the clamp is pinned byte by byte against float64."""
    from denoise_cases import RESOLVE_BYTES, RESOLVE_ROWS
    assert np.array_equal(O.resolve(RESOLVE_ROWS, math_mode=1), RESOLVE_BYTES)
    assert np.array_equal(O.resolve(RESOLVE_ROWS, math_mode=0), RESOLVE_BYTES)  # libm's pow is NaN for the negative mean: 0 as well
    # ordinary means, dense around the point where the clamp sets in (mean = 1: 255.5) and up to where the old conversion still worked
    m = np.concatenate([np.linspace(0.0, 1.2, 20001), np.exp(np.linspace(np.log(1.2), np.log(1e15), 2001))]).astype(np.float32)
    fb = np.stack([m, m * 2, m * 0.5, np.ones_like(m)], 1).astype(np.float32)
    fb[:, 0:3] *= 32
    fb[:, 3] = 32
    got = O.resolve(fb, math_mode=1)
    mean = fb[:, 0:3].astype(np.float64) / 32
    v = 255 * mean ** (1 / 2.2) + 0.5
    want = np.minimum(np.floor(v), 255)
    near = np.abs(v - np.round(v)) < 1e-3  # (within pow's 2e-6 relative error of a byte boundary: either neighbour)
    assert (np.abs(got[:, 0:3] - want) <= near).all() and (got[:, 3] == 255).all()
    assert near.mean() < 0.01 and (want == 255).mean() > 0.3 and len(np.unique(got[:, 0:3])) >= 250  # (the gamma curve is steep at 0: the grid steps over byte 1)


def test_libm_vs_detmath_image_tolerance():
    """The oracle in the reference's HOST math (libm) vs the deterministic math the GPU path uses: mean
    radiance within 1e-3 relative on a 128x72x16spp frame; most pixels are bit-identical, the rest are
    paths that a last-bit difference in a Lambert direction sent elsewhere."""
    tris = bunny_tris()
    cols, emis = position_colors(tris)
    sc = O.build_scene_from_triangles(tris, 256, cols, emis)
    rgba, hw, hh = O.decode_rgbe(hdr_bytes())
    w, h = 128, 72
    cam = probe_camera(sc.origin, sc.dps, 256, focus=9.0, lens_r=0.05)
    a, _, ca = sc.render_pt(O.HDRI(rgba, hw, hh, rgba, hw, hh, 0), cam, w, h, 0, math_mode=0, threads=8)
    b, _, cb = sc.render_pt(O.HDRI(rgba, hw, hh, rgba, hw, hh, 1), cam, w, h, 0, math_mode=1, threads=8)
    ma, mb = a[:, :3].astype(np.float64).mean(0), b[:, :3].astype(np.float64).mean(0)
    assert np.abs(ma - mb).max() / ma.max() < 1e-3
    assert (a == b).all(axis=1).mean() > 0.8
    assert abs(ca["rays"] - cb["rays"]) / ca["rays"] < 1e-3
