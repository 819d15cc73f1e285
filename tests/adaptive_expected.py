"""Expected buffers of steps under a sample mask (mvrt_pt_set_sample_mask) and the expected error mask (mvrt_pt_error_mask), from ORACLE primitives alone --
a helper, no test.

A step under a mask makes, for an ACTIVE pixel, exactly the additions an unmasked step makes, and none for an inactive one (include/mvrt.h "Adaptive
sampling").  So per iteration the whole frame's contributions are computed once -- the per-sample radiance from the oracle's render_pt( ..., want_samples=True ),
its 16 samples per pixel summed in ascending order from +0 in float32; the feature-buffer partial sums by the recipe of tests/aov_expected.py; the moment sums by
the recipe of tests/denoise_expected.py -- and added to the buffers of the active pixels only.  The error mask restates the header's formula, one explicit float32
operation at a time."""
import numpy as np

import aov_expected as A
import denoise_expected as D

f32 = np.float32
SPP = 16


class StepTerms:
    """what ONE iteration adds to every pixel of a W x H frame (global pixel order), and the statistics of its primary rays"""

    def __init__(self, O, sc, hdri, cam, W, H, iteration, aovs=True):
        _, sl, _ = sc.render_pt(hdri, cam, W, H, iteration, math_mode=1, want_samples=True, threads=8)
        self.samples = sl.reshape(W * H, SPP, 3)  # per-sample radiance
        rad = np.zeros((W * H, 3), f32)
        for s in range(SPP):  # ascending, one float32 addition at a time (np.sum adds pairwise)
            rad = (rad + self.samples[:, s]).astype(f32)
        self.radiance = rad
        self.s1, self.s2 = D.step_moments(sl)
        self.part_a = self.part_n = self.hit = None
        if aovs:
            ro, rd = A.primary_rays(O, cam, W, H, iteration)
            self.part_a, self.part_n, self.hit, _ = A.step_partials(O, sc, ro, rd)


_terms = {}


def step_terms(O, sc, hdri, cam, W, H, iteration, aovs=True):
    """StepTerms, computed once per (scene, camera, size, iteration): the tests share them and never modify them"""
    key = (id(sc), np.asarray(cam, f32).tobytes(), W, H, iteration)
    t = _terms.get(key, (None, None))[1]
    if t is None or (aovs and t.hit is None):
        t = StepTerms(O, sc, hdri, cam, W, H, iteration, aovs)
        _terms[key] = (sc, t)  # (the scene is kept, so that its id stays its own)
    return t


class Expected:
    """frame buffer, both feature buffers and moments of a W x H frame (all pixels, global order), accumulated step by step under masks"""

    def __init__(self, O, sc, hdri, W, H, aovs=True):
        self.O, self.sc, self.hdri, self.W, self.H, self.aovs = O, sc, hdri, W, H, aovs
        n = W * H
        self.fb = np.zeros((n, 4), f32)
        self.albedo = np.zeros((n, 4), f32)
        self.normal_depth = np.zeros((n, 4), f32)
        self.moments = np.zeros((n, 4), f32)
        self.steps = 0
        self.samples = None  # per-sample radiance of the last step in the compact numbering: (nActive * 16, 3)

    def step(self, cam, mask=None):
        """one step; mask: W * H entries (global pixel order), nonzero = active; None = every pixel.  Returns the step's StepTerms"""
        t = step_terms(self.O, self.sc, self.hdri, cam, self.W, self.H, self.steps, self.aovs)
        a = np.arange(self.W * self.H) if mask is None else np.nonzero(np.asarray(mask).reshape(-1))[0]
        self.fb[a, 0:3] = (self.fb[a, 0:3] + t.radiance[a]).astype(f32)
        self.fb[a, 3] = (self.fb[a, 3] + f32(SPP)).astype(f32)
        self.moments[a, 0] = (self.moments[a, 0] + t.s1[a]).astype(f32)
        self.moments[a, 1] = (self.moments[a, 1] + t.s2[a]).astype(f32)
        if self.aovs:
            self.albedo[a] = (self.albedo[a] + t.part_a[a]).astype(f32)
            self.normal_depth[a] = (self.normal_depth[a] + t.part_n[a]).astype(f32)
        self.samples = t.samples[a].reshape(-1, 3)
        self.steps += 1  # the iteration advances whether or not a pixel took part
        return t


def mask_statistics(t, mask):
    """of a step's active pixels: (share of valid pixels active, share of active samples whose primary ray hit, pixels partly covered, pixels that miss entirely)"""
    m = np.asarray(mask).reshape(-1) != 0
    per_pixel = t.hit[m].sum(1)
    return float(m.mean()), float(t.hit[m].mean()) if m.any() else 0.0, int(((per_pixel > 0) & (per_pixel < SPP)).sum()), int((per_pixel == 0).sum())


def error_mask(fb, moments, threshold, lum_floor=0.01, min_samples=32, max_samples=0):
    """mvrt_pt_error_mask on host arrays (n, 4) -> uint8 (n,).  n = fb.w; n < min: 1; max > 0 and n >= max: 0; else se = sqrt( var ) with the denoiser's var,
    1 iff se > threshold * max( m1, lum_floor )"""
    fb, moments = (np.ascontiguousarray(x, f32).reshape(-1, 4) for x in (fb, moments))
    n = fb[:, 3]
    ns = np.where(n == 0, f32(1), n).astype(f32)  # (placeholder: rule 1 decides those pixels)
    m1 = (moments[:, 0] / ns).astype(f32)
    m2 = (moments[:, 1] / ns).astype(f32)
    var = (D.fmax((m2 - (m1 * m1).astype(f32)).astype(f32), f32(0)) / D.fmax((ns - f32(1)).astype(f32), f32(1))).astype(f32)
    with np.errstate(invalid="ignore"):
        se = np.sqrt(var).astype(f32)
        noisy = se > (f32(threshold) * D.fmax(m1, f32(lum_floor))).astype(f32)
    capped = (n >= f32(max_samples)) if max_samples > 0 else np.zeros(len(n), bool)
    return np.where(n < f32(min_samples), 1, np.where(capped, 0, noisy)).astype(np.uint8)
