"""mvrt_denoise_buffers and mvrt_resolve_buffer on the hand-made frames of tests/denoise_cases.py -- sizes around the 32 x 8 tile, both parities of the ping-pong,
and the edges of the contract's arithmetic that a path-traced frame never visits -- against tests/denoise_expected.py (the numpy restatement of include/mvrt.h) and
the oracle's resolve.  Scratch and output are filled with bytes 0xFF before every call, so that a pixel left unwritten or a read of stale scratch shows as NaN."""
import numpy as np
import pytest

import denoise_cases as K
import denoise_expected as D
from fixtures import mv, O  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
f32 = np.float32


def run(mv, bufs, W, H, **params):
    """mvrt_denoise_buffers on device copies of `bufs`, with a caller's scratch of exactly the stated size; scratch and output start as 0xFF bytes; the inputs
    are checked to be unmodified afterwards"""
    devs = [mv.DeviceArray.from_host(b) for b in bufs]
    nbytes = mv.denoise_scratch_bytes(W, H)
    scratch = mv.DeviceArray.from_host(np.full(nbytes, 0xFF, np.uint8))
    out = mv.DeviceArray.from_host(np.full(W * H * 16, 0xFF, np.uint8).view(f32).reshape(W * H, 4))
    assert scratch.nbytes == nbytes and out.nbytes == W * H * 16
    mv.denoise_buffers(*devs, W, H, out, scratch, nbytes, **params)
    mv.synchronize()
    got = out.to_host()
    for d, b in zip(devs, bufs):
        assert np.array_equal(d.to_host().view(np.uint32), b.view(np.uint32)), "an input was modified"
    return got


def assert_same_where_finite(got, want, what):
    """NaN payloads and signs are not part of the contract: the same components are non-finite, and the finite ones are equal bit for bit"""
    bg, bw = ~np.isfinite(got), ~np.isfinite(want)
    assert np.array_equal(bg, bw), "%s: %d components non-finite on the device, %d in the helper, %d differ; first pixels %s" % (
        what, bg.sum(), bw.sum(), (bg != bw).sum(), np.nonzero((bg != bw).any(1))[0][:6])
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got == np.inf, want == np.inf), what
    D.assert_same(np.where(bg, f32(0), got), np.where(bw, f32(0), want), what)


@pytest.mark.parametrize("case", K.random_cases(), ids=K.case_id)
def test_random_frames_equal_the_contract(mv, O, case):
    """bit for bit against the float32 restatement; against the float64 evaluation of the same formula within four times what the float32 restatement itself
    differs from it (the device equals the restatement bit for bit, so it needs no margin of its own)"""
    W, H, params = case
    bufs = K.frame(W, H)
    got = run(mv, bufs, W, H, **params)
    D.assert_same(got, K.expected(O, bufs, W, H, params, "random"), K.case_id(case))
    err = K.rel_error(got, K.expected(O, bufs, W, H, params, "random", np.float64))
    print("%s: device against float64 %.3g (bound %.3g)" % (K.case_id(case), err, K.F32_AGAINST_F64_BOUND))
    assert err <= K.F32_AGAINST_F64_BOUND


@pytest.mark.parametrize("name", [n for n in K.SPECIAL_NAMES if n != "inf_radiance"])
def test_special_frames_equal_the_contract(mv, O, name):
    """33 x 9, 5 iterations.  negative_t is the frame that failed before the marker of "never a tap" moved out of geo.w: hit pixels with a negative t sum were
    neither filtered nor written, and came back as the 0xFF fill"""
    W, H = K.SPECIAL_SIZE
    bufs, params, info = K.special_frame(name)
    params = dict(params, iterations=5)
    got = run(mv, bufs, W, H, **params)
    want = K.expected(O, bufs, W, H, params, name)
    if info["finite"]:
        assert np.isfinite(want).all()
    if name == "all_empty":
        assert not got.view(np.uint32).any()
    if name == "all_sky":
        c = bufs[0]
        assert np.array_equal(got[:, 0:3], (c[:, 0:3] / c[:, 3:4]).astype(f32)) and (got[:, 3] == 1).all()
    if info["nan"]:
        assert_same_where_finite(got, want, name)
    else:
        D.assert_same(got, want, name)


@pytest.mark.parametrize("iterations", [1, 2, 5])
def test_infinite_radiance_stays_within_the_reach_of_the_taps(mv, O, iterations):
    """one hit pixel with +inf radiance: device and helper agree on which components are non-finite and bit for bit on the others; every non-finite pixel lies
    within Chebyshev distance 2 * ( 2^iterations - 1 ) of the bad one, and every pixel outside that reach has the bits it has without the +inf"""
    W, H = K.SPECIAL_SIZE
    bufs, params, info = K.special_frame("inf_radiance")
    params = dict(params, iterations=iterations)
    got = run(mv, bufs, W, H, **params)
    want = K.expected(O, bufs, W, H, params, "inf_radiance")
    assert_same_where_finite(got, want, "inf_radiance, %d iterations" % iterations)
    bx, by = info["bad"]
    ys, xs = (g.reshape(-1) for g in np.mgrid[0:H, 0:W])
    near = np.maximum(np.abs(xs - bx), np.abs(ys - by)) <= 2 * (2 ** iterations - 1)
    bad = ~np.isfinite(got).all(1)
    assert bad[by * W + bx] and not (bad & ~near).any(), np.nonzero(bad & ~near)[0]
    clean = [b.copy() for b in bufs]
    clean[0][by * W + bx, 0] = 1.0
    without = run(mv, clean, W, H, **params)
    D.assert_same(got[~near], without[~near], "outside the reach")
    assert (~near).sum() > 0 or iterations == 5


# ---- resolve ----------------------------------------------------------------------------------------------------------------------------------------
def resolve(mv, fb):
    d_in = mv.DeviceArray.from_host(np.ascontiguousarray(fb, f32))
    d_u8 = mv.DeviceArray.from_host(np.full((len(fb), 4), 0x5A, np.uint8))
    mv.resolve_buffer(d_in, len(fb), d_u8)
    mv.synchronize()
    return d_u8.to_host()


def test_resolve_outside_the_ordinary_range(mv, O):
    """NaN, negative means and 0 / 0 give 0; every mean whose scaled value is at least 255 gives 255, +inf and x / 0 included -- the promised bytes, and the oracle's"""
    got = resolve(mv, K.RESOLVE_ROWS)
    assert np.array_equal(got, K.RESOLVE_BYTES)
    assert np.array_equal(got, O.resolve(K.RESOLVE_ROWS, math_mode=1))


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_resolve_of_ordinary_buffers(mv, O, n):
    fb = K.resolve_ordinary(n)
    got = resolve(mv, fb)
    assert np.array_equal(got, O.resolve(fb, math_mode=1))
    assert n < 255 or (len(np.unique(got[:, 0:3])) > 100 and (got[:, 0:3] == 255).any() and (got[:, 0:3] < 64).any())


def test_a_denoised_empty_frame_resolves_to_black(mv, O):
    W, H = K.SPECIAL_SIZE
    bufs, params, _ = K.special_frame("all_empty")
    out = run(mv, bufs, W, H, **params)
    got = resolve(mv, out)
    assert np.array_equal(got, np.tile(np.array([0, 0, 0, 255], np.uint8), (W * H, 1)))
    assert np.array_equal(got, O.resolve(out, math_mode=1))
