"""Hand-made input frames of the denoiser (mvrt_denoise_buffers): seeded random frames that obey the buffers' own invariants, and named special frames at the
edges of the contract's arithmetic (include/mvrt.h "Denoiser: THE FILTER") -- a helper, no test.  tests/test_denoise_cpu.py runs the numpy restatement on them in
float32 and float64, tests/test_gpu_denoise_synthetic.py holds the GPU to the float32 one bit for bit.

A frame is built from per-pixel FIELDS and then assembled into the four float32 buffers (W * H, 4), one float32 operation at a time:
  n      samples, one of {16, 32, 64} (powers of two: sum / n is exact);  empty: about 5 % of the pixels have all four records 0
  h      hits, an integer in [0, n]: half of the pixels n, a tenth 0 (sky), the rest n * ( 1 - u^3 ) rounded
  a      albedo per channel in [0.05, 1]            albedo       = ( a * h, h )
  axis, sign  the hit normal, +-1 on one axis       normalDepth  = ( sign * h on axis, h * z ),  z in [2, 4]
  r      mean radiance per channel in [0, 4]        color        = ( n * r, n )
  var    in [0, 2]                                  moments      = ( n * lum( r ), n * ( lum( r )^2 + var ), 0, 0 )
Seven pixels in ten take z, the normal and r from smooth fields with one edge across the frame (so that taps get weights between 0 and 1), the rest are drawn
independently (so that the clamp of mvrt_exp and weights near 0 are visited too)."""
import numpy as np

import denoise_expected as D

f32 = np.float32
SIZES = [(1, 1), (1, 9), (9, 1), (31, 7), (32, 8), (33, 9), (65, 17), (37, 19)]  # around the 32 x 8 tile; 1 x 1: 16 B of records under the 256 B alignment of the scratch
OTHER_SIGMAS = dict(sigmaNormal=0.3, sigmaDepth=0.2, sigmaCoverage=0.6, sigmaLuminance=0.7, albedoFloor=0.2)
SPECIAL_SIZE = (33, 9)


def fields(W, H, seed=None):
    """the per-pixel fields of a random W x H frame (a dict of flat arrays, pixel = y * W + x)"""
    rng = np.random.RandomState(20260000 + 1000 * W + H if seed is None else seed)
    P = W * H
    y, x = (g.reshape(-1).astype(np.float64) for g in np.mgrid[0:H, 0:W])
    n = rng.choice([16, 32, 64], P).astype(np.float64)
    kind = rng.random_sample(P)
    h = np.where(kind < 0.5, n, np.where(kind < 0.6, 0.0, np.floor(n * (1 - rng.random_sample(P) ** 3) + 0.5)))
    empty = rng.random_sample(P) < 0.05
    side = (x * 0.6 + y > 0.45 * (W * 0.6 + H)).astype(np.float64)  # one edge across the frame
    free = rng.random_sample(P) < 0.3
    a = np.clip(np.array([0.5, 0.6, 0.4]) + side[:, None] * np.array([0.3, -0.3, 0.15]) + rng.normal(0, 0.03, (P, 3)), 0.05, 1.0)
    a = np.where(free[:, None], rng.uniform(0.05, 1.0, (P, 3)), a)
    z = np.where(free, rng.uniform(2.0, 4.0, P), 2.5 + (0.02 * x + 0.03 * y) % 0.5 + 0.6 * side)
    axis = np.where(free, rng.randint(0, 3, P), np.where(side > 0, 0, 2))
    sign = np.where(free, rng.choice([-1.0, 1.0], P), 1.0)
    smooth = np.stack([1.2 + np.sin(0.35 * x) + 0.8 * side, 1.0 + 0.6 * np.cos(0.5 * y), 0.8 + 0.5 * side], 1) + rng.normal(0, 0.25, (P, 3))
    r = np.where(free[:, None], rng.uniform(0.0, 4.0, (P, 3)), np.clip(smooth, 0.0, 4.0))
    var = rng.uniform(0.0, 2.0, P)
    return dict(W=W, H=H, n=n, h=h, empty=empty, a=a, z=np.clip(z, 2.0, 4.0), axis=axis, sign=sign, r=r, var=var)


def assemble(F):
    """fields -> (color, albedo, normalDepth, moments), float32 (W * H, 4) each"""
    P = F["W"] * F["H"]
    n, h = F["n"].astype(f32), F["h"].astype(f32)
    assert (h >= 0).all() and (h <= n).all() and (h == np.floor(h)).all()
    color, albedo, nd, mom = (np.zeros((P, 4), f32) for _ in range(4))
    r = F["r"].astype(f32)
    color[:, 0:3] = (n[:, None] * r).astype(f32)
    color[:, 3] = n
    albedo[:, 0:3] = (F["a"].astype(f32) * h[:, None]).astype(f32)
    albedo[:, 3] = h
    nd[np.arange(P), F["axis"].astype(int)] = (F["sign"].astype(f32) * h).astype(f32)
    nd[:, 3] = (h * F["z"].astype(f32)).astype(f32)
    l = D.lum(r[:, 0], r[:, 1], r[:, 2]).astype(f32)
    mom[:, 0] = (n * l).astype(f32)
    mom[:, 1] = (n * ((l * l).astype(f32) + F["var"].astype(f32)).astype(f32)).astype(f32)
    for b in (color, albedo, nd, mom):
        b[F["empty"]] = 0
    return color, albedo, nd, mom


_frames = {}


def frame(W, H):
    """the random frame of a size: built once, shared, read-only"""
    if (W, H) not in _frames:
        bufs = assemble(fields(W, H))
        for b in bufs:
            b.setflags(write=False)
        _frames[(W, H)] = bufs
    return _frames[(W, H)]


def random_cases():
    """[(W, H, params)]: every size with 1, 5 and 8 iterations (stride 128 exceeds every dimension), default parameters and NO_DEMODULATION; on 33 x 9 every
    iteration count (both parities of the ping-pong in front of the last iteration); on 37 x 19 one other set of sigmas"""
    out = []
    for W, H in SIZES:
        for it in (range(1, 9) if (W, H) == (33, 9) else (1, 5, 8)):
            out.append((W, H, dict(iterations=it)))
            out.append((W, H, dict(iterations=it, flags=D.NO_DEMODULATION)))
    out.append((37, 19, dict(OTHER_SIGMAS)))
    return out


def case_id(case):
    W, H, params = case[-3:]
    return "-".join([str(c) for c in case[:-3]] + ["%dx%d" % (W, H)] + ["%s%g" % (k[:6], v) for k, v in sorted(params.items())])


# ---- special frames ---------------------------------------------------------------------------------------------------------------------------------
def _exact_second_moment(mom, n):
    """moments.y = n * ( m1 * m1 ) with m1 = moments.x / n: n is a power of two, so m2 - m1 * m1 == 0 exactly"""
    m1 = (mom[:, 0] / n).astype(f32)
    return (n * (m1 * m1).astype(f32)).astype(f32)


def special(name, W=SPECIAL_SIZE[0], H=SPECIAL_SIZE[1]):
    """-> (buffers, params, info) of a named special frame.  info: {"finite": the helper's output is asserted finite, "nan": the contract's own arithmetic makes
    NaN on this frame (payloads and signs are not part of it), "bad": the pixel with the +inf (or None)}"""
    F = fields(W, H, seed=7 + 1000 * W + H)
    P = W * H
    y, x = (g.reshape(-1) for g in np.mgrid[0:H, 0:W])
    params, info = {}, dict(finite=True, bad=None, nan=False)
    post = None
    if name == "all_empty":
        F["empty"][:] = True
    elif name == "all_sky":
        F["empty"][:] = False
        F["h"][:] = 0
    elif name == "one_hit_in_sky":
        F["empty"][:] = False
        F["h"][:] = 0
        c = (H // 2) * W + W // 2
        F["h"][c] = F["n"][c]
    elif name == "checkerboard":  # hit and sky alternate: every tap of stride 1 in a diagonal direction is a hit, every axis neighbour is not
        F["empty"][:] = False
        F["h"] = np.where((x + y) % 2 == 0, np.maximum(F["h"], 1), 0.0)
    elif name == "var_zero":  # v == 0: sv = 1e-6, e = |dl| / 1e-6 reaches 1e6 and mvrt_exp clamps at -87
        def post(bufs):
            bufs[3][:, 1] = _exact_second_moment(bufs[3], np.where(F["empty"], 1, F["n"]).astype(f32))
    elif name == "var_clamped":  # m2 slightly below m1 * m1: max( m2 - m1 * m1, 0 )
        def post(bufs):
            bufs[3][:, 1] = (_exact_second_moment(bufs[3], np.where(F["empty"], 1, F["n"]).astype(f32)) * f32(1 - 1e-5)).astype(f32)
    elif name == "n_one":  # max( n - 1, 1 ) at n = 1
        F["n"][:] = 1
        F["h"] = (F["h"] > 0).astype(np.float64)
    elif name == "black_albedo":  # A = the floor on every hit pixel
        F["h"] = F["n"].copy()
        F["a"][:] = 0
    elif name == "tiny_floor":
        # black albedo, albedoFloor 1e-30: u reaches 4e30, lA * lA underflows to 0 and v = var / 0 = inf by the contract, so sv = inf and the luminance term is 0.
        # One iteration stays finite; from the second on, a tap whose w * w underflows to 0 (e > 43 from the other terms) adds 0 * inf = NaN to accv
        F["h"] = F["n"].copy()
        F["a"][:] = 0
        F["var"] = np.maximum(F["var"], 0.1)  # (var == 0 would make 0 / 0)
        params["albedoFloor"] = 1e-30
        info["finite"] = False
        info["nan"] = True
    elif name == "z_zero":
        F["z"][:] = 0
    elif name == "z_tiny":  # below the 1e-20f of max( max( Z_p, Z_q ), 1e-20f )
        F["z"] = F["z"] * 1e-25
    elif name == "z_huge":
        F["z"] = F["z"] * (1e30 / 3)
    elif name == "negative_t":  # a caller's t sums may be negative: the pixel is still n > 0 and h > 0, so it is filtered
        F["sign_t"] = np.where((x * 7 + y * 3) % 5 < 2, -1.0, 1.0)
        def post(bufs):
            bufs[2][:, 3] = (bufs[2][:, 3] * F["sign_t"].astype(f32)).astype(f32)
    elif name == "inf_radiance":
        c = (H // 2) * W + W // 2
        F["empty"][c] = False
        F["h"][c] = F["n"][c]
        info["bad"] = (W // 2, H // 2)
        info["finite"] = False
        info["nan"] = True
        def post(bufs):
            bufs[0][c, 0] = np.inf
    else:
        raise KeyError(name)
    bufs = assemble(F)
    if post:
        post(bufs)
    if name == "negative_t":
        neg = (bufs[2][:, 3] < 0) & (bufs[1][:, 3] > 0) & (bufs[0][:, 3] > 0)
        assert neg.sum() >= P // 5
    for b in bufs:
        b.setflags(write=False)
    return bufs, params, info


SPECIAL_NAMES = ["all_empty", "all_sky", "one_hit_in_sky", "checkerboard", "var_zero", "var_clamped", "n_one", "black_albedo", "tiny_floor", "z_zero", "z_tiny", "z_huge",
                 "negative_t", "inf_radiance"]

_specials = {}


def special_frame(name):
    if name not in _specials:
        _specials[name] = special(name)
    return _specials[name]


# ---- expected outputs, computed once and shared -----------------------------------------------------------------------------------------------------
_expected = {}


def expected(O, bufs, W, H, params, key, dtype=f32):
    """D.denoise of a frame, float32 (the contract) or float64 (the same formula as mathematics), cached by `key`; read-only"""
    k = (key, W, H, tuple(sorted(params.items())), np.dtype(dtype).name)
    if k not in _expected:
        out = D.denoise(O, *bufs, W, H, **params) if dtype is f32 else D.denoise(O, *bufs, W, H, dtype=dtype, exp=D.exp_f64, **params)
        out.setflags(write=False)
        _expected[k] = out
    return _expected[k]


def rel_error(a, b):
    """max over the rgb components of |a - b| / max( |b|, 1e-3 ), float64"""
    a, b = np.asarray(a, np.float64)[:, 0:3], np.asarray(b, np.float64)[:, 0:3]
    return float((np.abs(a - b) / np.maximum(np.abs(b), 1e-3)).max())


# max of rel_error( float32 helper, float64 helper ) over random_cases(), measured for this generator; the tests assert four times it, a margin for
# a change of the generator's seed -- the GPU equals the float32 helper bit for bit and needs none of its own
F32_AGAINST_F64 = 6.2e-6
F32_AGAINST_F64_BOUND = 4 * F32_AGAINST_F64

# ---- resolve (mvrt_resolve_buffer) outside the ordinary range: float4 rows and the bytes include/mvrt.h promises for them ------------------------------
RESOLVE_ROWS = np.array([[0, 0, 0, 0],                       # 0 / 0: black
                         [1, 1, 1, 0],                       # x / 0 = +inf: 255
                         [-1, 2, 3, 1],                      # a negative mean: 0; means above 1: 255
                         [np.inf, 1e15, 1e16, 1],            # 255 * pow + 0.5 = inf, 1.7e9 (below INT_MAX), 4.8e9 (above it)
                         [np.nan, 1e20, 3e38, 1],
                         [1, 1, 1, 1],                       # 255.5: the ordinary clamp
                         [1e-45, 1e-38, 1e-20, 1]], f32)     # a denormal, the smallest normals, a tiny mean: 255 * pow < 0.5
RESOLVE_BYTES = np.array([[0, 0, 0, 255], [255, 255, 255, 255], [0, 255, 255, 255], [255, 255, 255, 255], [0, 255, 255, 255], [255, 255, 255, 255], [0, 0, 0, 255]], np.uint8)


def resolve_ordinary(n, seed=5):
    """n float4 pixels of ordinary values: sums of 16 to 64 samples of radiance in [0, 3], one pixel in eight dark enough to land on the low bytes"""
    rng = np.random.RandomState(seed + n)
    w = rng.choice([16, 32, 48, 64], n).astype(f32)
    mean = rng.uniform(0.0, 3.0, (n, 3)) * np.where(rng.random_sample((n, 1)) < 0.125, 0.01, 1.0)
    return np.concatenate([(mean * w[:, None]).astype(f32), w[:, None]], 1).astype(f32)
