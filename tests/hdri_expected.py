"""What the HDRI importance tables and the importance sampler must give, computed in float64 with numpy: the formulas of HDRIstoreImportance
(voxKernel.cu:485-524) with float64 trigonometry, plain np.cumsum along both axes instead of the chunked f64 scan, and the inverse of the
sampler's direction mapping (renderCommon.hpp:354-365).  Table numbering as PathTracer.hdri_sat / HDRI.sat: 0 uniform, 1..6 = +x,-x,+y,-y,+z,-z."""
import numpy as np

AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
# the normals the tests sample with, by the table they select (k = 0.8, renderCommon.hpp:372-380); the diagonal selects the uniform table
NORMALS = np.vstack([np.full((1, 3), 3 ** -0.5), AXES]).astype(np.float32)


def solid_angles(w, h):
    """sr of the pixels of each row, float64 (h,)"""
    d_theta, d_phi = np.pi / h, 2.0 * np.pi / w
    theta = np.arange(h) * d_theta
    return 2.0 * np.sin(d_theta * 0.5) * np.sin(d_theta * 0.5 + theta) * d_phi


def importance(rgba, w, h, which):
    """lum * sr * wgt per pixel, float64 (h, w)"""
    px = np.asarray(rgba, np.float32).reshape(h, w, 4).astype(np.float64)
    lum = 0.2126 * px[:, :, 0] + 0.7152 * px[:, :, 1] + 0.0722 * px[:, :, 2]
    wgt = np.ones((h, w))
    if which > 0:
        d_theta, d_phi = np.pi / h, 2.0 * np.pi / w
        theta = np.arange(h) * d_theta
        s_y = 0.5 * (np.cos(theta) + np.cos(theta + d_theta))
        phi = d_phi * (np.arange(w) + 0.5) + np.pi
        sin_theta = np.sqrt(np.maximum(1.0 - s_y * s_y, 0.0))
        centre = np.stack([np.cos(phi)[None, :] * sin_theta[:, None], np.broadcast_to(s_y[:, None], (h, w)), np.sin(phi)[None, :] * sin_theta[:, None]], axis=-1)
        wgt = np.maximum(centre @ AXES[which - 1], 0.0)
    return lum * solid_angles(w, h)[:, None] * wgt


def normalised_table(rgba, w, h, which):
    """the summed-area table as a fraction of its total, float64 (h, w); all zeros where there is no total"""
    c = np.cumsum(np.cumsum(importance(rgba, w, h, which), axis=1), axis=0)
    return c / c[-1, -1] if c[-1, -1] > 0 else np.zeros_like(c)


def pixel_of_direction(d, w, h):
    """the pixel a direction falls into, float64: (x, y)"""
    d = np.asarray(d, np.float64)
    phi = np.arctan2(d[2], d[0]) + np.pi
    theta = np.arctan2(np.hypot(d[0], d[2]), d[1])
    return min(int(phi / (2.0 * np.pi) * w), w - 1), min(int(theta / np.pi * h), h - 1)


def count(table, w, h, x, y):
    """the table's share of pixel (x, y) in units of 2^-32, as the sampler's getCount takes it from the u32 table (wrapping u32 arithmetic)"""
    t = np.asarray(table, np.uint32).reshape(h, w).astype(np.int64)
    a = t[y - 1, x - 1] if x > 0 and y > 0 else 0
    b = t[y - 1, x] if y > 0 else 0
    c = t[y, x - 1] if x > 0 else 0
    return int(((t[y, x] - b) % 2 ** 32 + (a - c) % 2 ** 32) % 2 ** 32)


def stratified_u(n, seed):
    """(n * n, 4) float32: (u0, u1) one jittered point per cell of an n x n grid, (u2, u3) in [0.05, 0.95] -- clear of the pixel's borders"""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    u = np.empty((n * n, 4), np.float32)
    u[:, 0] = ((i.ravel() + rng.random(n * n)) / n).astype(np.float32)
    u[:, 1] = ((j.ravel() + rng.random(n * n)) / n).astype(np.float32)
    u[:, 2:] = (0.05 + 0.9 * rng.random((n * n, 2))).astype(np.float32)
    return np.minimum(u, np.float32(1.0 - 2.0 ** -24))
