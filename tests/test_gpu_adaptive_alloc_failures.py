"""Every device allocation of mvrt_pt_set_sample_mask is made to fail in turn (mvrt_test_fail_allocation): on the first call of a frame, where no mask is in
force, and on a later one, where one is.  The call returns an error, the mask that was in force (or none) stays in force -- a step afterwards still matches
tests/adaptive_expected.py bit for bit -- and mvrt_test_allocation_state shows no leaked buffer."""
import gc

import numpy as np
import pytest

import adaptive_expected as X
from alloc_sweep import mv  # noqa: F401 (the fixture)
from common import bunny_tris, hdr_bytes, position_colors, probe_camera
from fixtures import O  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

W, H = 64, 36
f32 = np.float32


@pytest.fixture(autouse=True)
def no_buffer_outlives_its_handles(mv):
    gc.collect()
    before = mv.allocation_state()[0]
    yield
    mv.set_test_fail_allocation(0)
    gc.collect()
    assert mv.allocation_state()[0] == before  # every handle of the test is destroyed: nothing is left


def live(mv):
    return mv.allocation_state()[0]


def fail_nth(mv, n, call):
    """arm, call, and see the call fail on exactly that allocation; returns the change of the number of live buffers"""
    before = live(mv)
    mv.set_test_fail_allocation(n)
    with pytest.raises(mv.MvrtError, match="mvrt_test_fail_allocation"):
        call()
    assert mv.lib().mvrt_test_fail_allocation(0) == 0  # (it has disarmed itself; this is for a test that fails above)
    return live(mv) - before


def count_allocations(mv, call):
    t0 = mv.allocation_state()[2]
    call()
    n = mv.allocation_state()[2] - t0
    assert n >= 1
    return n


def test_failed_set_sample_mask_keeps_the_mask_in_force(mv, O):
    tris = bunny_tris()
    cols, emis = position_colors(tris)
    sc = O.build_scene_from_triangles(tris, 256, cols, emis)
    rgba, hw, hh = O.decode_rgbe(hdr_bytes())
    Hd = O.HDRI(rgba, hw, hh, rgba, hw, hh, math_mode=1)
    cam = probe_camera(sc.origin, sc.dps, 256, focus=9.0, lens_r=0.05)
    n = W * H
    rng = np.random.default_rng(3)
    A, B = rng.random(n) < 0.4, rng.random(n) < 0.7

    def handle():
        pt = mv.PathTracer()
        pt.setup(None)
        pt.set_moments(True)
        pt.resizeFrameBufferIfNeeded(None, W, H)
        pt.loadHDRIPixels(None, rgba, hw, hh, rgba, hw, hh)
        pt.m_intersectorOctreeGPU.upload(sc.nodes, sc.attrs, sc.origin, sc.dps, sc.grid_res, sc.has_emission)
        return pt

    def check(pt, exp, what):
        for got, want in ((pt.read_framebuffer(), exp.fb), (pt.read_moments(), exp.moments)):
            assert np.array_equal(got[:n].view(np.uint32), want.view(np.uint32)), what
            assert not got[n:].any()

    # the masks live in device arrays of the test's own (mvrt_malloc is the caller's memory and passes the hook by)
    dA, dB = (mv.DeviceArray.from_host(np.concatenate([m, np.zeros(256, bool)])[: (n + 255) // 256 * 256].astype(np.uint8)) for m in (A, B))
    probe = handle()
    first = count_allocations(mv, lambda: probe.set_sample_mask(dA))
    later = count_allocations(mv, lambda: probe.set_sample_mask(dB))
    print("allocations of set_sample_mask: first call %d, later call %d" % (first, later))
    assert later >= 1  # a later call allocates too: its list is built aside
    del probe

    pt = handle()
    exp = X.Expected(O, sc, Hd, W, H, aovs=False)
    pt.step(None, cam)
    exp.step(cam)
    pt.join(None)  # (the deferred step is launched now, with its slot's traversal workspace: the hook below meets the allocations of set_sample_mask alone)
    for k in range(1, first + 1):  # no mask in force: none afterwards
        assert fail_nth(mv, k, lambda: pt.set_sample_mask(dA)) == 0, k
        assert pt.active_pixels() == n
    pt.step(None, cam)
    exp.step(cam)
    check(pt, exp, "after the failed first calls")
    held = live(mv)
    assert pt.set_sample_mask(dA) == A.sum()
    assert live(mv) == held + 1  # the list; the scratch is gone
    for k in range(1, later + 1):  # mask A in force: still A afterwards
        assert fail_nth(mv, k, lambda: pt.set_sample_mask(dB)) == 0, k
        assert pt.active_pixels() == A.sum()
    pt.step(None, cam)
    exp.step(cam, A)
    check(pt, exp, "after the failed later calls")
    held = live(mv)  # (with the traversal workspaces the steps since have made)
    assert pt.set_sample_mask(dB) == B.sum() and live(mv) == held  # the new list replaced the old one
    pt.step(None, cam)
    exp.step(cam, B)
    check(pt, exp, "mask B")
    assert pt.getSteps() == 4
