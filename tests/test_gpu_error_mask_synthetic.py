"""mvrt_pt_error_mask on hand-made frame-buffer and moments arrays, copied into the handle's own buffers (the handle is the only way in), against
tests/adaptive_expected.error_mask, which restates the formula of include/mvrt.h ("Adaptive sampling").  The path tracer only ever produces sample counts that are
multiples of 16 and moments of non-negative radiance; a caller who gathers buffers from other ranks, or resumes a frame, may hold anything."""
import numpy as np
import pytest

import adaptive_expected as X
from fixtures import mv  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
f32 = np.float32

# valid pixels: 1, 255, 256, 257 (a partial last wave behind whole ones) and 100 x 37
FRAMES = [(1, 1), (51, 5), (16, 16), (257, 1), (100, 37)]
# (threshold, lumFloor, minSamples, maxSamples)
PARAMS = [(0.5, 0.01, 2, 64), (0.5, 0.01, 1, 0), (0.05, 0.5, 16, 32)]
UP = np.nextafter(f32(2.5), f32(3))
# (n, moments.x, moments.y), cycled over the pixels; under PARAMS[0]:
RECIPES = [(1, 1.0, 3.0),                      # n == minSamples - 1: 1;  under PARAMS[1] it is max( n - 1, 1 ) at n = 1
           (2, 2.0, 2.5),                      # n == minSamples and an exact tie: m1 = 1, var = 0.25, se = 0.5 == 0.5 * 1 -> 0 (the comparison is strict)
           (2, 2.0, UP),                       # the same with one ulp more on moments.y -> 1
           (63, 63 * 0.7, 63 * 50.49),         # n == maxSamples - 1, noisy: 1
           (64, 64 * 0.7, 64 * 50.49),         # n == maxSamples: 0 whatever the moments say
           (0, 0.0, 0.0),                      # no samples: 1
           (32, 32 * 0.9, 32 * 0.81 * (1 - 1e-4)),   # m2 below m1 * m1: the clamp, se = 0 -> 0
           (32, 32 * 0.001, 32 * (1e-6 + 1.24e-4)),  # m1 below lumFloor: se = 0.002 is above threshold * m1 and below threshold * lumFloor -> 0
           (32, 32 * 0.02, 32 * (4e-4 + 31 * 4e-4)), # m1 above lumFloor: se = 0.02 > 0.01 -> 1
           (32, -16.0, 32 * 3.25),             # a negative m1: max( m1, lumFloor ) = lumFloor -> 1
           (32, -16.0, 32 * 0.25),             # ... and with var == 0 -> 0
           (48, 48 * 1.5, 48 * (2.25 + 0.3)),
           (16, 16 * 0.2, 16 * (0.04 + 40.0))]
NON_FINITE = [(32, np.inf, 1.0), (32, 1.0, np.inf), (32, np.nan, 1.0), (32, 1.0, np.nan), (32, np.inf, np.inf), (32, -np.inf, 1.0), (np.inf, 1.0, 1.0), (np.nan, 1.0, 1.0),
              (32, 3e38, 3e38), (32, 1.0, 2.0)]


def handle(mv, w, h):
    pt = mv.PathTracer()
    pt.setup(None)
    pt.set_moments(True)
    pt.resizeFrameBufferIfNeeded(None, w, h)
    return pt


def fill(mv, pt, valid, recipes, seed):
    """frame buffer and moments of the handle from the recipes (cycled from a per-frame offset, radiance random); the padding of the owned-pixel layout is set to
    records that WOULD be active (no samples) and to noisy ones: it must never count.  Returns the host copies of the valid part"""
    owned = pt.owned_pixels()
    assert owned >= valid and owned % 256 == 0
    rng = np.random.RandomState(seed)
    r = np.array([recipes[(i + seed) % len(recipes)] for i in range(owned)], f32)
    fb = np.concatenate([rng.uniform(0, 4, (owned, 3)).astype(f32) * r[:, 0:1], r[:, 0:1]], 1).astype(f32)
    mo = np.zeros((owned, 4), f32)
    mo[:, 0:2] = r[:, 1:3]
    fb[valid:] = np.where((np.arange(owned - valid) % 2 == 0)[:, None], f32(0), np.array([32, 32, 32, 32], f32))
    mo[valid:] = np.array([32, 32 * 50.0, 0, 0], f32)
    for dst, src in ((pt.framebuffer_dev(), fb), (pt.moments_dev(), mo)):
        d = mv.DeviceArray.from_host(src)
        mv.memcpy_d2d(dst, d, owned * 16)
        mv.synchronize()
    assert np.array_equal(pt.read_framebuffer().view(np.uint32), fb.view(np.uint32)) and np.array_equal(pt.read_moments().view(np.uint32), mo.view(np.uint32))
    return fb[:valid], mo[:valid]


def check(mv, pt, valid, fb, mo, params):
    threshold, floor, lo, hi = params
    with np.errstate(all="ignore"):
        want = X.error_mask(fb, mo, threshold, floor, lo, hi)
    d = mv.DeviceArray.from_host(np.full(pt.owned_pixels(), 0xFF, np.uint8))
    out, count = pt.error_mask(threshold, lum_floor=floor, min_samples=lo, max_samples=hi, out_dev=d)
    got = d.to_host()
    assert np.array_equal(got[:valid], want), (params, np.nonzero(got[:valid] != want)[0][:8])
    assert not got[valid:].any(), "padding"
    assert count == int(want.sum()), (count, int(want.sum()))
    return want


@pytest.mark.parametrize("w,h", FRAMES)
def test_error_mask_on_hand_made_buffers(mv, w, h):
    valid = w * h
    pt = handle(mv, w, h)
    fb, mo = fill(mv, pt, valid, RECIPES, seed=w)
    for params in PARAMS:
        want = check(mv, pt, valid, fb, mo, params)
        assert valid < 255 or 0 < want.sum() < valid
    if valid >= len(RECIPES):
        # the recipes decide what their comments say, under the parameters they were written for (the helper is held to the header's text here, not only the GPU to it)
        with np.errstate(all="ignore"):
            want = X.error_mask(fb, mo, *PARAMS[0])
        first = {(i + w) % len(RECIPES): i for i in reversed(range(len(RECIPES)))}  # recipe -> a pixel that holds it
        assert [int(want[first[k]]) for k in range(11)] == [1, 0, 1, 1, 0, 1, 0, 0, 1, 1, 0]
        with np.errstate(all="ignore"):
            assert X.error_mask(fb, mo, *PARAMS[1])[first[0]] == 1  # n = 1: var = ( 3 - 1 ) / max( 0, 1 ) = 2, se = 1.41 > 0.5


@pytest.mark.parametrize("ones", [True, False])
def test_error_mask_all_ones_and_all_zeros_at_257_pixels(mv, ones):
    """five waves, the last with one lane in use: the per-wave count adds up to 257, or nothing is added at all"""
    pt = handle(mv, 257, 1)
    fb, mo = fill(mv, pt, 257, [(0, 0.0, 0.0)] if ones else [(64, 64 * 0.7, 64 * 50.49)], seed=3)
    want = check(mv, pt, 257, fb, mo, PARAMS[0])
    assert want.sum() == (257 if ones else 0)


def test_error_mask_with_non_finite_moments(mv):
    """inf and NaN in the moments and in the sample count: the bytes are what the formula's comparisons give (a comparison with NaN is false)"""
    pt = handle(mv, 51, 5)
    fb, mo = fill(mv, pt, 255, NON_FINITE, seed=0)
    sums = [int(check(mv, pt, 255, fb, mo, params).sum()) for params in PARAMS]
    assert 0 < sums[0] < 255 and 0 < sums[1] < 255, sums  # (an infinite second moment is noisy, a finite noisy pixel among them is too; the rest compare false)
