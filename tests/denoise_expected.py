"""Expected luminance moments (mvrt_pt_set_moments) and the expected output of the a-trous denoiser (mvrt_denoise_buffers / mvrt_pt_denoise) -- a helper, no test.

Both restate the text of include/mvrt.h ("Luminance moments", "Denoiser: THE FILTER"), not the kernels: every operation is one explicit float32 operation in
the order that text gives, sums are sequential additions (np.sum adds pairwise), exp is the oracle's mvrt_exp (oracle.detmath("exp")), division and sqrt are
numpy's IEEE float32 ones.  The per-sample radiance comes from the oracle's render_pt( ..., want_samples=True )."""
import numpy as np

f32 = np.float32
SPP = 16
DEFAULTS = dict(iterations=5, sigmaNormal=0.5, sigmaDepth=0.05, sigmaCoverage=0.25, sigmaLuminance=2.0, albedoFloor=0.01, flags=0)
NO_DEMODULATION = 1
KERNEL = [f32(0.0625), f32(0.25), f32(0.375), f32(0.25), f32(0.0625)]


def lum(r, g, b, dtype=f32):
    """( 0.2126f * r + 0.7152f * g ) + 0.0722f * b; the constants are the float32 ones in every dtype"""
    t = dtype
    return ((t(f32(0.2126)) * r).astype(t) + (t(f32(0.7152)) * g).astype(t)).astype(t) + (t(f32(0.0722)) * b).astype(t)


def fmax(a, b, dtype=f32):
    """a < b ? b : a"""
    return np.where(a < b, b, a).astype(dtype)


def exp_f64(x):
    """mvrt_exp as mathematics: the argument clamped to [-87, 88], then the exponential"""
    return np.exp(np.clip(x, -87.0, 88.0))


def step_moments(samples):
    """(s1, s2) per pixel of one step from its (n * 16, 3) per-sample radiance: the 16 samples in ascending order from +0, l * l rounded before it is added"""
    s = np.ascontiguousarray(samples, f32).reshape(-1, SPP, 3)
    n = len(s)
    s1 = np.zeros(n, f32)
    s2 = np.zeros(n, f32)
    for k in range(SPP):
        l = lum(s[:, k, 0], s[:, k, 1], s[:, k, 2]).astype(f32)
        s1 = (s1 + l).astype(f32)
        s2 = (s2 + (l * l).astype(f32)).astype(f32)
    return s1, s2


class ExpectedMoments:
    """the moments buffer of a W x H frame (all pixels, global order), accumulated step by step"""

    def __init__(self, W, H):
        self.W, self.H = W, H
        self.moments = np.zeros((W * H, 4), f32)

    def step(self, samples):
        s1, s2 = step_moments(samples)
        self.moments[:, 0] = (self.moments[:, 0] + s1).astype(f32)
        self.moments[:, 1] = (self.moments[:, 1] + s2).astype(f32)
        return s1, s2


def prepare(color, albedo, normal_depth, moments, albedoFloor, flags, dtype=f32):
    """-> dict of per-pixel arrays (flat, W * H): c (n, 3), A (n, 3), u (n, 3), N (n, 3), Z, f, v, valid (n > 0 and h > 0), sky (n > 0 and h == 0), empty (n == 0).
    dtype: the precision of every operation (the float32 buffers and the float32 constants converted to it exactly); float32 is the contract"""
    t = dtype
    color, albedo, normal_depth, moments = (np.ascontiguousarray(a, f32).reshape(-1, 4).astype(t) for a in (color, albedo, normal_depth, moments))
    n = color[:, 3]
    h = albedo[:, 3]
    empty = n == 0
    ns = np.where(empty, t(1), n).astype(t)  # (placeholders keep the arithmetic of unused pixels finite; their results are masked out)
    hs = np.where(h == 0, t(1), h).astype(t)
    with np.errstate(all="ignore"):
        c = (color[:, 0:3] / ns[:, None]).astype(t)
        if flags & NO_DEMODULATION:
            A = np.ones_like(c)
        else:
            miss = (ns - h).astype(t)
            A = fmax(((albedo[:, 0:3] + miss[:, None]).astype(t) / ns[:, None]).astype(t), t(f32(albedoFloor)), t)
        u = (c / A).astype(t)
        N = (normal_depth[:, 0:3] / ns[:, None]).astype(t)
        Z = (normal_depth[:, 3] / hs).astype(t)
        f = (h / ns).astype(t)
        m1 = (moments[:, 0] / ns).astype(t)
        m2 = (moments[:, 1] / ns).astype(t)
        var = (fmax((m2 - (m1 * m1).astype(t)).astype(t), t(0), t) / fmax((ns - t(1)).astype(t), t(1), t)).astype(t)
        lA = lum(A[:, 0], A[:, 1], A[:, 2], t).astype(t)
        v = (var / (lA * lA).astype(t)).astype(t)
    valid = ~empty & (h > 0)
    return dict(c=c, A=A, u=u, N=N, Z=Z, f=f, v=v, valid=valid, sky=~empty & (h == 0), empty=empty)


def denoise(O, color, albedo, normal_depth, moments, W, H, dtype=f32, exp=None, **params):
    """the contract on host arrays -> (W * H, 4) of `dtype`; O = the oracle module (for mvrt_exp).  Also returns nothing else: see prepare() for the statistics.
    dtype / exp: float32 and None (the oracle's mvrt_exp) are the contract; np.float64 and exp_f64 evaluate the same formula as mathematics, for a cross-check"""
    t = dtype
    if exp is None:
        assert t is f32, "mvrt_exp is a float32 function: pass exp= with another dtype"
        exp = lambda x: O.detmath("exp", x.astype(f32).reshape(-1)).reshape(x.shape)
    P = dict(DEFAULTS)
    P.update(params)
    pr = prepare(color, albedo, normal_depth, moments, P["albedoFloor"], int(P["flags"]), t)
    sn2 = t(t(f32(P["sigmaNormal"])) * t(f32(P["sigmaNormal"])))
    sz, sf, sl = t(f32(P["sigmaDepth"])), t(f32(P["sigmaCoverage"])), t(f32(P["sigmaLuminance"]))
    valid = pr["valid"].reshape(H, W)
    N = pr["N"].reshape(H, W, 3)
    Z = pr["Z"].reshape(H, W)
    f = pr["f"].reshape(H, W)
    u = pr["u"].reshape(H, W, 3).copy()
    v = pr["v"].reshape(H, W).copy()
    ys, xs = np.mgrid[0:H, 0:W]
    for i in range(int(P["iterations"])):
        s = 1 << i
        with np.errstate(all="ignore"):
            lp = lum(u[..., 0], u[..., 1], u[..., 2], t).astype(t)
            sv = ((sl * np.sqrt(v).astype(t)).astype(t) + t(f32(1e-6))).astype(t)
        acc = np.zeros((H, W, 3), t)
        accv = np.zeros((H, W), t)
        ws = np.zeros((H, W), t)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qy, qx = ys + dy * s, xs + dx * s
                inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                qyc, qxc = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                take = inside & valid[qyc, qxc] & valid
                Nq, Zq, fq, uq, vq = N[qyc, qxc], Z[qyc, qxc], f[qyc, qxc], u[qyc, qxc], v[qyc, qxc]
                with np.errstate(all="ignore"):
                    d = (N - Nq).astype(t)
                    e = (((d[..., 0] * d[..., 0]).astype(t) + (d[..., 1] * d[..., 1]).astype(t)).astype(t) + (d[..., 2] * d[..., 2]).astype(t)).astype(t)
                    e = (e / sn2).astype(t)
                    dz = ((Z - Zq).astype(t) / (sz * fmax(fmax(Z, Zq, t), t(f32(1e-20)), t)).astype(t)).astype(t)
                    e = (e + (dz * dz).astype(t)).astype(t)
                    df = ((f - fq).astype(t) / sf).astype(t)
                    e = (e + (df * df).astype(t)).astype(t)
                    lq = lum(uq[..., 0], uq[..., 1], uq[..., 2], t).astype(t)
                    e = (e + (np.abs((lp - lq).astype(t)).astype(t) / sv).astype(t)).astype(t)
                    e = np.where(take, e, t(0)).astype(t)
                    ex = exp((-e).astype(t))
                    w = (t(KERNEL[dy + 2] * KERNEL[dx + 2]) * ex).astype(t)
                    acc = np.where(take[..., None], (acc + (w[..., None] * uq).astype(t)).astype(t), acc)
                    accv = np.where(take, (accv + ((w * w).astype(t) * vq).astype(t)).astype(t), accv)
                    ws = np.where(take, (ws + w).astype(t), ws)
        with np.errstate(all="ignore"):
            un = (acc / ws[..., None]).astype(t)
            vn = (accv / (ws * ws).astype(t)).astype(t)
        u = np.where(valid[..., None], un, u).astype(t)
        v = np.where(valid, vn, v).astype(t)
    out = np.zeros((H * W, 4), t)
    A = pr["A"]
    k = pr["valid"]
    with np.errstate(all="ignore"):
        out[k, 0:3] = (u.reshape(-1, 3)[k] * A[k]).astype(t)
    out[k, 3] = 1
    k = pr["sky"]
    out[k, 0:3] = pr["c"][k]
    out[k, 3] = 1
    return out


def assert_same(got, want, what):
    """bit equality of two float32 (n, 4) buffers, pixel by pixel"""
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(1))[0]
    assert len(bad) == 0, "%s: %d of %d pixels differ, first %s: %s vs %s" % (what, len(bad), len(got), bad[:4], got[bad[:2]], want[bad[:2]])


def rel_mse(a, b, mask=None):
    """mean( |a - b|^2 / ( |b|^2 + 1e-2 ) ) over the pixels (rgb vectors), float64"""
    a = np.asarray(a, np.float64)[:, 0:3]
    b = np.asarray(b, np.float64)[:, 0:3]
    r = ((a - b) ** 2).sum(1) / ((b ** 2).sum(1) + 1e-2)
    return float(r.mean() if mask is None else r[mask].mean())
