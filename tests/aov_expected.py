"""Expected first-hit feature buffers (MVRT_AOV_ALBEDO, MVRT_AOV_NORMAL_DEPTH) from ORACLE primitives alone -- a helper, no test.

Sampler, camera and traversal come from a provider; the default provider is the oracle.  Per sample the primary ray is rebuilt the way the path tracer generates it (spp = iteration * 16 + localSpp, stream = murmur( 0, pixel ), PMJ dimension 0 =
pixel jitter, dimension 1 = lens sample, thin-lens camera), all rays go through ONE Scene.trace, and the sums are explicit sequential float32 additions in
the order include/mvrt.h states: per pixel and step the 16 samples in ascending order starting from +0, then that partial sum onto the buffer.
tests/test_aov_cpu.py pins the rebuilt rays to the oracle's own path tracer (they hit exactly where render_pt's primary rays hit)."""
import numpy as np

f32 = np.float32
SPP = 16


class OracleProvider:
    """where the ray construction takes its sampler, camera and traversal from: the default is the oracle.  tests/test_gpu_reference_pins.py passes one over
    the compiled reference instead (reference_pins.ReferenceProvider), so that the expected buffers do not go through the oracle's restatement of them."""

    def __init__(self, O):
        self.O = O
        self.R = O.RenderOracle(0)  # sample2d and the camera hold no transcendental: the math mode does not matter

    def sample2d(self, sample_idx, dim, stream):
        """PMJSampler::sample2d per element: (n,) uint32 each -> (n, 2) float32"""
        return self.R.sample2d(self.O.pmj_table(), sample_idx, dim, stream)

    def shoot_thin_lens(self, cam, px, fl):
        """CameraPinhole::shootThinLens: px (n, 4) int32 x, y, W, H; fl (n, 4) float32 xo, yo, u0, u1 -> ro, rd"""
        return self.R.camera_shoot(cam, px, fl, True)

    def trace(self, sc, ro, rd):
        """-> {"t", "nMajor", "vIndex"}; a miss keeps t = MAX_FLOAT"""
        return sc.trace(ro, rd, threads=8)


def primary_rays(O, cam, W, H, iteration, pixels=None, provider=None):
    """(ro, rd) of the 16 primary rays of every pixel in `pixels` (global pixel indices; default: the whole frame), (n * 16, 3) float32 each"""
    provider = OracleProvider(O) if provider is None else provider
    pixels = np.asarray(range(W * H) if pixels is None else pixels, np.int64)
    n = len(pixels)
    stream = np.repeat(np.array([O.murmur(0, [int(p)]) for p in pixels], np.uint32), SPP)  # MurmurHash32( 0 ).combine( pixelIdx ): pinned by tests/test_oracle_pins.py
    spp = np.tile(np.arange(iteration * SPP, (iteration + 1) * SPP, dtype=np.uint32), n)
    u = provider.sample2d(spp, np.zeros(n * SPP, np.uint32), stream)  # dimension 0: the pixel jitter
    l = provider.sample2d(spp, np.ones(n * SPP, np.uint32), stream)  # dimension 1: the lens sample
    p = np.repeat(pixels, SPP)
    px = np.stack([p % W, p // W, np.full(n * SPP, W), np.full(n * SPP, H)], 1).astype(np.int32)
    return provider.shoot_thin_lens(cam, px, np.concatenate([u, l], 1).astype(f32))


def step_partials(O, sc, ro, rd, provider=None):
    """one step's partial sums per pixel from its n * 16 primary rays -> (partA (n, 4), partN (n, 4), hit (n, 16) bool, normal (n, 16, 3))"""
    provider = OracleProvider(O) if provider is None else provider
    n = len(ro) // SPP
    h = provider.trace(sc, ro, rd)
    hit = (h["t"] != O.MAX_FLOAT).reshape(n, SPP)
    t = h["t"].reshape(n, SPP)
    nm = h["nMajor"].reshape(n, SPP)
    vi = h["vIndex"].reshape(n, SPP)
    d = rd.reshape(n, SPP, 3)
    colour = sc.attrs[np.where(hit, vi, 0), 0:3].astype(f32) / f32(255)  # rawReflectance: channel / 255.0f
    normal = np.zeros((n, SPP, 3), f32)
    for major, axis in ((1, 0), (2, 1), (0, 2)):  # nMajor 1: x, 2: y, 0: z; the normal faces the ray
        sel = hit & (nm == major)
        normal[..., axis][sel] = np.where(f32(0) < d[..., axis][sel], f32(-1), f32(1))
    part_a = np.zeros((n, 4), f32)
    part_n = np.zeros((n, 4), f32)
    for s in range(SPP):  # ascending spp, one float32 addition at a time (np.sum adds pairwise); a miss adds nothing
        m = hit[:, s]
        part_a[m, 0:3] = part_a[m, 0:3] + colour[m, s]
        part_a[m, 3] = part_a[m, 3] + f32(1)
        part_n[m, 0:3] = part_n[m, 0:3] + normal[m, s]
        part_n[m, 3] = part_n[m, 3] + t[m, s]
    return part_a, part_n, hit, normal


class Expected:
    """the two buffers of a W x H frame (all pixels, global order), accumulated step by step"""

    def __init__(self, O, sc, W, H, provider=None):
        self.O, self.sc, self.W, self.H = O, sc, W, H
        self.provider = OracleProvider(O) if provider is None else provider
        self.albedo = np.zeros((W * H, 4), f32)
        self.normal_depth = np.zeros((W * H, 4), f32)
        self.steps = 0

    def step(self, cam, iteration=None):
        """add one step (iteration = steps so far unless given); returns (hit (n, 16), normal (n, 16, 3)) of this step for statistics"""
        it = self.steps if iteration is None else iteration
        ro, rd = primary_rays(self.O, cam, self.W, self.H, it, provider=self.provider)
        pa, pn, hit, normal = step_partials(self.O, self.sc, ro, rd, self.provider)
        self.albedo = self.albedo + pa
        self.normal_depth = self.normal_depth + pn
        self.steps += 1
        return hit, normal


def frame_statistics(hit, normal):
    """what the GPU tests assert about their inputs: share of samples that hit, pixels with some but not all 16 samples hitting, set of normals seen"""
    per_pixel = hit.sum(1)
    seen = set(map(tuple, normal[hit].astype(int).tolist()))
    return float(hit.mean()), int(((per_pixel > 0) & (per_pixel < SPP)).sum()), seen


def encode_albedo(albedo_sum, samples):
    """apps/rtcamp_batch --aov: byte = (int)( 255 * ( sum / samples ) + 0.5f ), in fp32 in this order; alpha 255"""
    v = (f32(255) * (albedo_sum[:, 0:3] / samples[:, None]).astype(f32)).astype(f32) + f32(0.5)
    return v.astype(f32).astype(np.int32).astype(np.uint8)


def encode_normal(normal_sum, samples):
    """byte = (int)( 255 * ( 0.5f * ( sum / samples ) + 0.5f ) + 0.5f )"""
    m = (normal_sum[:, 0:3] / samples[:, None]).astype(f32)
    v = (f32(255) * ((f32(0.5) * m).astype(f32) + f32(0.5)).astype(f32)).astype(f32) + f32(0.5)
    return v.astype(f32).astype(np.int32).astype(np.uint8)
