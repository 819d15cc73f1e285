"""Environment maps for the HDRI tests: seeded numpy, float32 RGBA of shape (h * w, 4), alpha 1, row-major from the zenith row down (row 0 is
theta = 0, +y).  Every map is a pure function of its arguments, so the CPU and the GPU tests see the same pixels."""
import numpy as np

f32 = np.float32


def _rgba(rgb, w, h):
    out = np.ones((h, w, 4), f32)
    out[:, :, :3] = rgb
    return np.ascontiguousarray(out.reshape(h * w, 4))


def noise(w, h, seed=1):
    """random RGB in [0.1, 1.1): no zero pixel"""
    rng = np.random.default_rng(seed)
    return _rgba(rng.random((h, w, 3), dtype=f32) + f32(0.1), w, h)


def black_ground(w, h, seed=2):
    """noise sky over a ground hemisphere (the lower half of the rows) that is exactly 0: the -y table has no total"""
    px = noise(w, h, seed).reshape(h, w, 4)
    px[h // 2:, :, :3] = 0.0
    return np.ascontiguousarray(px.reshape(h * w, 4))


def all_black(w, h):
    return _rgba(f32(0.0), w, h)


def constant(w, h, value=1.0):
    return _rgba(f32(value), w, h)


def sun(w, h):
    """a 1e-3 sky with a 2x2 block of 5e4: almost all of every table's range lies in four pixels"""
    px = np.full((h, w, 3), 1e-3, f32)
    x, y = w // 3, h // 4
    px[y:y + 2, x:x + 2] = f32(5e4)
    return _rgba(px, w, h)


def denormal_floor(w, h, seed=3):
    """black but for a band of rows around the horizon at 0.5e-38 .. 1e-38 (below the smallest normal f32, 1.18e-38): the pixels,
    their luminance and every lum * sr * wgt are f32 denormals, and nothing larger is there to hide them -- a table build that flushes f32
    denormals gets seven zero tables here.  The band spans the horizon, so all seven tables have a total."""
    rng = np.random.default_rng(seed)
    px = np.zeros((h, w, 3), f32)
    y0, y1 = h // 2 - max(h // 8, 1), h // 2 + max(h // 8, 1)
    px[y0:y1] = (f32(1e-38) * (f32(0.5) + f32(0.5) * rng.random((y1 - y0, w, 3), dtype=f32))).astype(f32)
    assert (px[y0:y1] > 0).all() and (px < f32(1.17549435e-38)).all()
    return _rgba(px, w, h)


def encode_rgbe_flat(rgba, w, h):
    """a flat (not run-length encoded) Radiance .hdr file of the map: the bytes whose decoding is value = c * 2^(E-136)"""
    rgb = np.asarray(rgba, f32).reshape(h * w, 4)[:, :3].astype(np.float64)
    m = rgb.max(axis=1)
    _, e = np.frexp(m)  # m = f * 2^e, 0.5 <= f < 1
    scale = np.where(m > 1e-32, np.ldexp(256.0, -e), 0.0)
    out = np.zeros((h * w, 4), np.uint8)
    out[:, :3] = np.minimum(rgb * scale[:, None], 255.0).astype(np.uint8)
    out[:, 3] = np.where(m > 1e-32, e + 128, 0).astype(np.uint8)
    return b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (h, w) + out.tobytes()
