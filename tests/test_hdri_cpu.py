"""The environment light on the CPU oracle, beyond the one 64x32 map of the other tests: importance tables of maps wider and taller than one
512-entry scan chunk against a float64 reference (the first pin of the oracle's chunked scan and its carry), the importance sampler against the
nearest lookup and the tables it sampled from, tables without a total (the defined deviation: they are all zeros and select nothing, include/mvrt.h
at mvrt_pt_load_hdri), and maps with a huge dynamic range.  tests/test_gpu_hdri_maps.py holds the device to this oracle bit for bit."""
import numpy as np
import pytest

import hdri_expected as E
import hdri_maps as M
from oracle import oracle as O

TABLE_SIZES = [(64, 32), (513, 3), (3, 513), (1025, 2), (520, 260), (1030, 515)]
# Largest |table / 2^32 - float64 reference| of the oracle in math mode 0 (libm) over TABLE_SIZES and all seven tables, as measured: 2.02e-7
# (at 3x513; 1.9e-7 at 1025x2, 0.8e-7 to 1.1e-7 at the other sizes; the deterministic math set of mode 1 gives the same to two digits).  The terms are f32 products of three factors and two f32 sines and the u32 entry
# truncates (2.3e-10), so errors of a few 1e-7 of full scale are the formats' own.  The bound is twice the measured value.  A wrong or missing
# carry moves every entry behind the first chunk by that chunk's weight -- 1e-1 of full scale at these sizes.
TABLE_MEASURED = 2.02e-7
TABLE_BOUND = 2 * TABLE_MEASURED


@pytest.fixture(scope="module")
def maps():
    cache = {}

    def get(kind, w, h):
        if (kind, w, h) not in cache:
            cache[(kind, w, h)] = getattr(M, kind)(w, h)
        return cache[(kind, w, h)]
    return get


@pytest.mark.parametrize("w,h", TABLE_SIZES)
def test_tables_against_float64_cumsum(maps, w, h):
    """All seven tables of the oracle, in both math modes, against lum * sr * wgt in float64 summed with np.cumsum: |table / 2^32 - reference| <=
    TABLE_BOUND = 4.04e-7 of full scale (twice the 2.02e-7 measured in mode 0, see above), every row non-decreasing from left to right and every column from
    top to bottom (the last row and the column differences are what the sampler searches).  Widths and heights of 513, 520, 1025 and 1030 take
    the scan through two and three chunks in each direction; 64x32 is the size every other test uses."""
    rgba = maps("noise", w, h)
    worst = {}
    for mode in (0, 1):
        H = O.HDRI(rgba, w, h, rgba, w, h, math_mode=mode)
        for which in range(7):
            got = H.sat(which).reshape(h, w)
            want = E.normalised_table(rgba, w, h, which)
            assert want[-1, -1] == 1.0  # no zero table among these
            worst[mode] = max(worst.get(mode, 0.0), float(np.abs(got.astype(np.float64) / 2.0 ** 32 - want).max()))
            g = got.astype(np.int64)
            assert (np.diff(g, axis=1) >= 0).all() and (np.diff(g, axis=0) >= 0).all(), (mode, which)
            assert got[-1, -1] == 0xFFFFFFFF
    print("largest table deviation %dx%d: libm %.3g, deterministic set %.3g" % (w, h, worst[0], worst[1]))
    assert worst[0] <= TABLE_BOUND and worst[1] <= TABLE_BOUND, worst


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("w,h", [(64, 32), (520, 260)])
def test_importance_sample_agrees_with_nearest_lookup_and_table(maps, w, h, mode):
    """For N over the six axes and a diagonal (all seven tables) and a 32x32 stratified (u0, u1) grid: the radiance returned is exactly what the
    nearest lookup of the lighting map gives for the returned direction, and pdf = count(X, Y) / 2^32 / sr for the pixel (X, Y) that the direction
    falls into by float64 spherical coordinates, count read from the table as the sampler's getCount does.  (u2, u3) stay 5 % clear of the pixel's
    borders, and no case has to be left out.  Tolerance of the pdf: it is an f32 quotient of (float)count / 2^32 and sr = 2 sin(a) sin(b) dPhi with
    f32 sines of f32 arguments; the check takes float64 sines of the same f32 arguments, so what is left are about eight f32 roundings (two sines
    of <= 2 ulp each, three products, the conversion, two quotients): 8 * 2^-24 = 4.8e-7, bound 1e-6 relative."""
    rgba = maps("noise", w, h)
    H = O.HDRI(rgba, w, h, rgba, w, h, math_mode=mode)
    tables = [H.sat(i) for i in range(7)]
    px = rgba.reshape(h, w, 4)
    f32 = np.float32
    d_theta, d_phi = f32(3.14159265) / f32(h), f32(2.0) * f32(3.14159265) / f32(w)
    worst = 0.0
    for which, N in enumerate(E.NORMALS):
        for u in E.stratified_u(32, 100 + which):
            d, L, pdf = H.importance_sample(N, u)
            assert np.array_equal(L, H.sample_nearest(d, False)), (which, u)
            x, y = E.pixel_of_direction(d, w, h)
            assert np.array_equal(L, px[y, x, :3] * f32(1.75)), (which, u, x, y)
            theta = f32(y) * d_theta
            a, b = f32(d_theta * f32(0.5)), f32(d_theta * f32(0.5) + theta)
            sr = 2.0 * np.sin(float(a)) * np.sin(float(b)) * float(d_phi)
            want = E.count(tables[which], w, h, x, y) / 2.0 ** 32 / sr
            assert want > 0
            worst = max(worst, abs(float(pdf) - want) / want)
    print("largest relative pdf deviation %dx%d mode %d: %.3g" % (w, h, mode, worst))
    assert worst <= 1e-6


ZERO_TABLE_MAPS = [
    ("black_ground", 64, 32, {4}),          # a sky over a black ground: nothing to sample for a surface that faces down
    ("all_black", 8, 4, set(range(7))),
    ("constant", 1, 1, {2, 3, 4, 6}),        # the one pixel centre looks along +x on the horizon
    ("constant", 2, 1, {3, 4}),
    ("constant", 1, 2, {2, 6}),
]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kind,w,h,zero", ZERO_TABLE_MAPS)
def test_zero_tables_are_zero_and_select_nothing(maps, kind, w, h, zero, mode):
    """A table whose total is not > 0 is stored as all zeros, and importance_sample on it returns (N, 0, 1) -- direction N, no radiance, pdf 1 --
    for every u; every other table of the same map has its full range and samples with a finite pdf > 0.  Which tables are zero is part of the pin."""
    rgba = maps(kind, w, h)
    H = O.HDRI(rgba, w, h, rgba, w, h, math_mode=mode)
    us = E.stratified_u(4, 7)
    for which, N in enumerate(E.NORMALS):
        t = H.sat(which)
        if which in zero:
            assert not t.any(), which
            for u in us:
                d, L, pdf = H.importance_sample(N, u)
                assert np.array_equal(d, N) and not L.any() and pdf == 1.0, (which, u)
        else:
            assert t[-1] == 0xFFFFFFFF, which
            for u in us:
                d, L, pdf = H.importance_sample(N, u)
                assert np.isfinite(pdf) and pdf > 0 and np.isfinite(d).all() and np.isfinite(L).all(), (which, u, pdf)
                assert abs(float(np.linalg.norm(d.astype(np.float64))) - 1.0) < 1e-5


@pytest.mark.parametrize("kind", ["sun", "denormal_floor"])
def test_no_bad_pdf_on_hard_maps(maps, kind):
    """20 000 seeded samples (N among the six axes and the diagonal, u uniform in [0, 1)^4) of the sun map (5e4 in a 2x2 block on a 1e-3 sky) and
    the denormal-floor map (nothing but f32 denormals) at 520x260: no pdf is non-finite or <= 0, in either math mode."""
    w, h = 520, 260
    rgba = maps(kind, w, h)
    rng = np.random.default_rng(11)
    us = rng.random((20000, 4), dtype=np.float32)
    ns = E.NORMALS[rng.integers(0, 7, 20000)]
    for mode in (0, 1):
        H = O.HDRI(rgba, w, h, rgba, w, h, math_mode=mode)
        assert all(H.sat(i)[-1] == 0xFFFFFFFF for i in range(7))
        pdf = np.array([H.importance_sample(n, u)[2] for n, u in zip(ns, us)])
        assert np.isfinite(pdf).all() and (pdf > 0).all(), (mode, pdf[~(np.isfinite(pdf) & (pdf > 0))][:5])
