"""The stream-order tests (tests/test_gpu_stream_order.py) without a GPU: every declaration of include/mvrt.h with a `stream` parameter is named by a case of the
table, the helper kernel cross-compiles for gfx950, and every case's real and decoy inputs are valid, differ, and have different answers in the CPU models."""
import os
import re

import numpy as np
import pytest

import streams as SH
import test_gpu_stream_order as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_hipcc = pytest.mark.skipif(not os.path.exists(SH.HIPCC), reason="no hipcc")


def stream_taking_declarations():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvrt.h")).read(), flags=re.S)
    decls = re.findall(r"\bint\s+(mvrt_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
    return [name for name, args in decls if re.search(r"\bvoid\s*\*\s*\*?\s*stream\b", args)]


def test_every_stream_taking_declaration_is_named_by_a_case():
    names = stream_taking_declarations()
    assert len(names) > 80 and "mvrt_svo_surface_smooth" in names and "mvrt_pt_step" in names, "the header was not parsed: %d declarations" % len(names)
    assert len(T.EXEMPT) == 6 and set(T.EXEMPT) == {"mvrt_stream_create", "mvrt_stream_destroy", "mvrt_stream_synchronize", "mvrt_memcpy_h2d", "mvrt_memcpy_d2h",
                                                     "mvrt_memcpy_d2d"}
    assert set(T.EXEMPT) <= set(names)
    covered = {a for c in T.CASES for a in c.apis}
    missing = [n for n in names if n not in covered and n not in T.EXEMPT]
    assert not missing, "no case of tests/test_gpu_stream_order.py makes these calls on a held stream: %s" % " ".join(missing)
    unknown = sorted(a for a in covered if a not in names)
    assert not unknown, "cases name entry points the header does not declare with a stream: %s" % " ".join(unknown)
    assert "mvrt_memcpy_d2d" in covered  # exempt as the harness's tool, and still a case of its own


def test_case_names_are_unique_and_every_case_names_its_pin():
    names = [c.name for c in T.CASES]
    assert len(set(names)) == len(names)
    for c in T.CASES:
        assert c.pinned, c.name


@needs_hipcc
def test_hold_kernel_compiles_for_gfx950(tmp_path):
    assert os.path.getsize(SH.compile_hold(tmp_path)) > 0  # -Wall -Werror


def test_hold_is_within_the_clamp_of_the_kernel():
    assert 0 < SH.HOLD_MS <= SH.MAX_HOLD_MS and SH.CALIBRATION_HOLD_MS <= SH.MAX_HOLD_MS
    src = open(SH.SOURCE).read()
    assert "#define SH_MAX_MS %du" % SH.MAX_HOLD_MS in src and "SH_MAX_ITERATIONS" in src and "asm" not in src


def test_decoys_are_valid_inputs_and_differ_from_the_real_ones():
    for xyz, at in (T.SET1, T.SET2, T.SET3):
        assert xyz.dtype == np.uint32 and xyz.shape == (T.N_VOXELS, 3) and xyz.max() < T.RES and len(np.unique(T.morton(xyz))) == T.N_VOXELS
        assert at.shape == (T.N_VOXELS, 8) and at.dtype == np.uint8
    assert not np.array_equal(np.sort(T.morton(T.SET1[0])), np.sort(T.morton(T.SET2[0])))
    for a, b in zip(T.RAYS, T.DECOY_RAYS):
        assert a.shape == b.shape == (T.N_RAYS,) and a.dtype == b.dtype and np.isfinite(a.astype(np.float64)).all() and not np.array_equal(a, b)
    codes = set(T.morton(T.SET1[0]).tolist()) | {0xFFFFFFFFFFFFFFFF}
    assert set(T.hints(1).tolist()) <= codes and set(T.hints(2).tolist()) <= codes and not np.array_equal(T.hints(1), T.hints(2))
    for k in (0, 1):
        m = T.masks(k)
        assert m.shape == (T.N_VOXELS,) and m.max() < 64
        q = T.queries(k)
        assert np.abs(q).max() <= 1 << 22
        s = T.sample_mask(k, 256)
        assert s.shape == (256,) and s[: T.W * T.H].any() and not s[T.W * T.H:].any()
        v, c, e = T.triangles(bool(k))
        lo, hi = T.VS.LOWER, T.VS.LOWER + T.EXTENT
        assert len(v) % 3 == 0 and (v >= lo).all() and (v <= hi).all() and c.shape == v.shape == e.shape
        assert np.isfinite(T.camera(k)).all() and all(np.isfinite(m).all() for m in T.look_at(k))
        assert all(np.isfinite(b).all() for b in T.denoise_frame(101 + k))
    fv, fd = T.faces_of(T.SET1[0])
    assert len(fv) == 600 and fv.max() < T.N_VOXELS and fd.max() < 6
    (a, b), (c, d) = T.ao_inputs()
    assert not np.array_equal(a, b) and sorted(zip(a.tolist(), c.tolist())) == sorted(zip(b.tolist(), d.tolist()))
    assert not np.array_equal(T.masks(0), T.masks(1)) and not np.array_equal(T.queries(0), T.queries(1)) and not np.array_equal(T.flags(0), T.flags(1))
    assert not np.array_equal(T.sample_mask(0, 256), T.sample_mask(1, 256)) and not np.array_equal(T.camera(0), T.camera(1))
    assert not np.array_equal(T.triangles(False)[0], T.triangles(True)[0])


MODELLED = [c for c in T.CASES if c.cpu]


def test_every_case_has_a_model_or_says_why_not():
    for c in T.CASES:
        assert bool(c.cpu) != bool(c.no_model), c.name
    assert sorted(c.name for c in T.CASES if not c.cpu) == sorted(
        ["trace_batch", "trace_batch_hinted", "trace_batch_range", "trace_batch_cone", "render_primary", "render_primary_lod", "resolve_buffer", "denoise_buffers",
         "surface_ao", "surface_merged_masked", "download", "lod_prepare", "build", "build_ex", "build_synthetic"] + [c.name for c in T.CASES if c.name.startswith("pt_")])


@pytest.mark.parametrize("c", MODELLED, ids=[c.name for c in MODELLED])
def test_the_cpu_model_answers_differ_between_real_and_decoy(c):
    real, decoy = T.stated(c.cpu(0)), T.stated(c.cpu(1))
    assert len(real) == len(decoy) and len(real) >= 1
    for a in real + decoy:
        a = np.asarray(a)
        assert a.dtype.kind in "iufb", (c.name, a.dtype)
    assert not T.same(real, decoy), "%s: expected(real) == expected(decoy)" % c.name
