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


def lum(r, g, b):
    """( 0.2126f * r + 0.7152f * g ) + 0.0722f * b"""
    return ((f32(0.2126) * r).astype(f32) + (f32(0.7152) * g).astype(f32)).astype(f32) + (f32(0.0722) * b).astype(f32)


def fmax(a, b):
    """a < b ? b : a"""
    return np.where(a < b, b, a).astype(f32)


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


def prepare(color, albedo, normal_depth, moments, albedoFloor, flags):
    """-> dict of per-pixel arrays (flat, W * H): c (n, 3), A (n, 3), u (n, 3), N (n, 3), Z, f, v, valid (n > 0 and h > 0), sky (n > 0 and h == 0), empty (n == 0)"""
    color, albedo, normal_depth, moments = (np.ascontiguousarray(a, f32).reshape(-1, 4) for a in (color, albedo, normal_depth, moments))
    n = color[:, 3]
    h = albedo[:, 3]
    empty = n == 0
    ns = np.where(empty, f32(1), n).astype(f32)  # (placeholders keep the arithmetic of unused pixels finite; their results are masked out)
    hs = np.where(h == 0, f32(1), h).astype(f32)
    c = (color[:, 0:3] / ns[:, None]).astype(f32)
    if flags & NO_DEMODULATION:
        A = np.ones_like(c)
    else:
        miss = (ns - h).astype(f32)
        A = fmax(((albedo[:, 0:3] + miss[:, None]).astype(f32) / ns[:, None]).astype(f32), f32(albedoFloor))
    u = (c / A).astype(f32)
    N = (normal_depth[:, 0:3] / ns[:, None]).astype(f32)
    Z = (normal_depth[:, 3] / hs).astype(f32)
    f = (h / ns).astype(f32)
    m1 = (moments[:, 0] / ns).astype(f32)
    m2 = (moments[:, 1] / ns).astype(f32)
    var = (fmax((m2 - (m1 * m1).astype(f32)).astype(f32), f32(0)) / fmax((ns - f32(1)).astype(f32), f32(1))).astype(f32)
    lA = lum(A[:, 0], A[:, 1], A[:, 2]).astype(f32)
    v = (var / (lA * lA).astype(f32)).astype(f32)
    valid = ~empty & (h > 0)
    return dict(c=c, A=A, u=u, N=N, Z=Z, f=f, v=v, valid=valid, sky=~empty & (h == 0), empty=empty)


def denoise(O, color, albedo, normal_depth, moments, W, H, **params):
    """the contract on host arrays -> (W * H, 4) float32; O = the oracle module (for mvrt_exp).  Also returns nothing else: see prepare() for the statistics"""
    P = dict(DEFAULTS)
    P.update(params)
    pr = prepare(color, albedo, normal_depth, moments, P["albedoFloor"], int(P["flags"]))
    sn2 = f32(f32(P["sigmaNormal"]) * f32(P["sigmaNormal"]))
    sz, sf, sl = f32(P["sigmaDepth"]), f32(P["sigmaCoverage"]), f32(P["sigmaLuminance"])
    valid = pr["valid"].reshape(H, W)
    N = pr["N"].reshape(H, W, 3)
    Z = pr["Z"].reshape(H, W)
    f = pr["f"].reshape(H, W)
    u = pr["u"].reshape(H, W, 3).copy()
    v = pr["v"].reshape(H, W).copy()
    ys, xs = np.mgrid[0:H, 0:W]
    for i in range(int(P["iterations"])):
        s = 1 << i
        lp = lum(u[..., 0], u[..., 1], u[..., 2]).astype(f32)
        with np.errstate(invalid="ignore"):
            sv = ((sl * np.sqrt(v).astype(f32)).astype(f32) + f32(1e-6)).astype(f32)
        acc = np.zeros((H, W, 3), f32)
        accv = np.zeros((H, W), f32)
        ws = np.zeros((H, W), f32)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qy, qx = ys + dy * s, xs + dx * s
                inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                qyc, qxc = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                take = inside & valid[qyc, qxc] & valid
                Nq, Zq, fq, uq, vq = N[qyc, qxc], Z[qyc, qxc], f[qyc, qxc], u[qyc, qxc], v[qyc, qxc]
                with np.errstate(all="ignore"):
                    d = (N - Nq).astype(f32)
                    e = (((d[..., 0] * d[..., 0]).astype(f32) + (d[..., 1] * d[..., 1]).astype(f32)).astype(f32) + (d[..., 2] * d[..., 2]).astype(f32)).astype(f32)
                    e = (e / sn2).astype(f32)
                    dz = ((Z - Zq).astype(f32) / (sz * fmax(fmax(Z, Zq), f32(1e-20))).astype(f32)).astype(f32)
                    e = (e + (dz * dz).astype(f32)).astype(f32)
                    df = ((f - fq).astype(f32) / sf).astype(f32)
                    e = (e + (df * df).astype(f32)).astype(f32)
                    lq = lum(uq[..., 0], uq[..., 1], uq[..., 2]).astype(f32)
                    e = (e + (np.abs((lp - lq).astype(f32)).astype(f32) / sv).astype(f32)).astype(f32)
                    e = np.where(take, e, f32(0)).astype(f32)
                    ex = O.detmath("exp", (-e).astype(f32).reshape(-1)).reshape(H, W)
                    w = (f32(KERNEL[dy + 2] * KERNEL[dx + 2]) * ex).astype(f32)
                    acc = np.where(take[..., None], (acc + (w[..., None] * uq).astype(f32)).astype(f32), acc)
                    accv = np.where(take, (accv + ((w * w).astype(f32) * vq).astype(f32)).astype(f32), accv)
                    ws = np.where(take, (ws + w).astype(f32), ws)
        with np.errstate(all="ignore"):
            un = (acc / ws[..., None]).astype(f32)
            vn = (accv / (ws * ws).astype(f32)).astype(f32)
        u = np.where(valid[..., None], un, u).astype(f32)
        v = np.where(valid, vn, v).astype(f32)
    out = np.zeros((H * W, 4), f32)
    A = pr["A"]
    k = pr["valid"]
    out[k, 0:3] = (u.reshape(-1, 3)[k] * A[k]).astype(f32)
    out[k, 3] = 1
    k = pr["sky"]
    out[k, 0:3] = pr["c"][k]
    out[k, 3] = 1
    return out


def rel_mse(a, b, mask=None):
    """mean( |a - b|^2 / ( |b|^2 + 1e-2 ) ) over the pixels (rgb vectors), float64"""
    a = np.asarray(a, np.float64)[:, 0:3]
    b = np.asarray(b, np.float64)[:, 0:3]
    r = ((a - b) ** 2).sum(1) / ((b ** 2).sum(1) + 1e-2)
    return float(r.mean() if mask is None else r[mask].mean())
