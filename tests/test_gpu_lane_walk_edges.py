"""The per-lane octree walk of include/mvrt/device.hpp on the MI355X, on the adversarial rays of the reference pins: user kernels on the unlimited and the limited
methods (tests/hip/device_api_probe.hip, tests/hip/range_probe.hip; the thread's own stack in scratch memory and the caller's stack in LDS), mvrt_trace_batch_range
(kTraceRange, stack in LDS), occluded() and the occlusion bake -- against the expectations of tests/lane_walk_expected.py, which tests/test_lane_walk_cpu.py holds the
host build of the same header to: R.rays_of plus 160 000 far-origin rays per scene, the oracle bit for bit, unlimited and under the limit cycle of tests/test_gpu_range.py,
the t = +inf hits of rays without a direction under MAX_FLOAT (a miss) and +inf (a hit).  bunny64, deep14 and deep16 (16 levels: the deepest the view accepts), uploaded
embedded and plain; the deep scenes also built by the library, so that its own kids, masks and psumCold arrays are walked.  mvrt_trace_batch rides along: the stream
kernel on the same rays.  No launch has more than 250 000 rays: the ray set goes in two parts."""
import ctypes as C

import numpy as np
import pytest

import deep_scenes as D
import lane_walk_expected as E
from fixtures import mv, O  # noqa: F401 (fixtures)
from rays import compile_probe, compile_range_probe, expected_open, oracle_t, probe_range, probe_trace

pytestmark = pytest.mark.gpu

RAGGED = (1, 63, 65)  # batch sizes around the 64-lane block of kTraceRange, cycled over the first 20 000 rays
N_RAGGED = 20_000


@pytest.fixture(scope="module")
def probes(mv, tmp_path_factory):
    d = tmp_path_factory.mktemp("lane_walk_probes")
    return compile_probe(d, []), compile_range_probe(d, [])


def in_parts(exp, call):
    """call( slice ) -> {output: array} on [0, n_set) and [n_set, n), joined"""
    cuts = (slice(0, exp.n_set), slice(exp.n_set, len(exp.ro)))
    assert all(0 < c.stop - c.start <= 250_000 for c in cuts)
    parts = [call(c) for c in cuts]
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def make_octree(mv, exp, how):
    sc = exp.sc
    svo = mv.IntersectorOctreeGPU()
    if how == "uploaded":
        svo.upload(sc.nodes, sc.attrs, sc.origin, sc.dps, sc.grid_res, sc.has_emission, embeddedMask=exp.embedded)
    else:
        s = exp.rs.deep
        svo.build_voxels(s.xyz, s.attrs, origin=s.origin, dps=s.dps, gridRes=s.res, flags=0 if exp.embedded else 2)
    view = svo.device_view()
    assert view.flavour == (0 if exp.embedded else 1) and view.levels == exp.rs.levels and view.structBytes == C.sizeof(mv.DeviceOctree)
    assert np.array_equal(np.array(view.lower[:], np.float32), exp.rs.lower) and np.array_equal(np.array(view.upper[:], np.float32), exp.rs.upper)
    return svo, view


CASES = [(scene, how, embedded) for scene in ("bunny64", "deep14", "deep16") for how in ("uploaded", "built") for embedded in (True, False)
         if how == "uploaded" or scene.startswith("deep")]


@pytest.mark.parametrize("scene,how,embedded", CASES, ids=["%s-%s-%s" % (s, h, "embedded" if e else "plain") for s, h, e in CASES])
def test_every_walk_equals_the_oracle(mv, O, probes, scene, how, embedded):
    trace_probe, range_probe = probes
    exp = E.expectation(O, scene, embedded)
    exp.check_populations()
    svo, view = make_octree(mv, exp, how)
    # unlimited: the stream kernel, then the device API in both stack modes
    exp.check_unlimited(in_parts(exp, lambda c: svo.intersect(exp.ro[c], exp.rd[c], exp.sh[c], want_descents=True)), "mvrt_trace_batch")
    for mode in (0, 1):
        exp.check_unlimited(in_parts(exp, lambda c: probe_trace(mv, trace_probe, view, exp.ro[c], exp.rd[c], exp.sh[c], mode)), "intersectEx, stack mode %d" % mode)
    # limited: kTraceRange, then the device API in both stack modes with occluded()
    got = [in_parts(exp, lambda c: svo.intersect_range(exp.ro[c], exp.rd[c], exp.tmax[c], exp.sh[c], want_descents=True))]
    exp.check_limited(got[0], "mvrt_trace_batch_range", occluded=False)
    for mode in (0, 1):
        got.append(in_parts(exp, lambda c: probe_range(mv, range_probe, view, exp.ro[c], exp.rd[c], exp.sh[c], exp.tmax[c], mode)))
        exp.check_limited(got[-1], "intersectRangeEx, stack mode %d" % mode)
    assert np.array_equal(got[0]["descents"], got[1]["descents"]) and np.array_equal(got[1]["descents"], got[2]["descents"])


@pytest.mark.parametrize("scene,how,embedded", CASES, ids=["%s-%s-%s" % (s, h, "embedded" if e else "plain") for s, h, e in CASES])
def test_ragged_batches(mv, O, scene, how, embedded):
    """the first 20 000 rays again in batches of 1, 63 and 65 rays: partly filled blocks of the library's kernels"""
    exp = E.expectation(O, scene, embedded)
    svo, _ = make_octree(mv, exp, how)
    start, i, unlimited, limited = 0, 0, [], []
    while start < N_RAGGED:
        c = slice(start, min(start + RAGGED[i % 3], N_RAGGED))
        unlimited.append(svo.intersect(exp.ro[c], exp.rd[c], exp.sh[c], want_descents=True))
        limited.append(svo.intersect_range(exp.ro[c], exp.rd[c], exp.tmax[c], exp.sh[c], want_descents=True))
        start, i = c.stop, i + 1
    for k in E.OUTPUTS:
        assert np.array_equal(E.R.bits(np.concatenate([b[k] for b in unlimited])), E.R.bits(exp.want[k][:N_RAGGED])), k
    for k in ("t", "nMajor", "vIndex"):
        assert np.array_equal(E.R.bits(np.concatenate([b[k] for b in limited])), E.R.bits(exp.exp[k][:N_RAGGED])), k
    de = np.concatenate([b["descents"] for b in limited])
    keep = exp.keep[:N_RAGGED]
    assert np.array_equal(de[keep], exp.want["descents"][:N_RAGGED][keep]) and (de <= exp.want["descents"][:N_RAGGED]).all()


def test_occlusion_bake_at_16_levels(mv, O):
    """kSurfaceAo on 2 048 faces of deep16, spread over the face list of mvrt_svo_surface_mesh (clusters and isolated voxels), 16 rays each, within 4 voxels
    and without a limit: the open counts of the oracle's unlimited t of the bake's own rays"""
    exp = E.expectation(O, "deep16", True)
    svo, view = make_octree(mv, exp, "built")
    dps = np.float32(view.dps)
    mesh = svo.surface_mesh()
    pick = np.linspace(0, len(mesh["faceVoxel"]) - 1, 2048).astype(np.int64)
    fv, fd = np.ascontiguousarray(mesh["faceVoxel"][pick]), np.ascontiguousarray(mesh["faceDir"][pick])
    assert len(np.unique(pick)) == 2048 and set(fd.tolist()) == set(range(6))
    xyz, _ = svo.read_voxels()
    t = oracle_t(mv, exp.sc, xyz, fv, fd, 16)
    t.setflags(write=False)
    dfv, dfd = mv.DeviceArray.from_host(fv), mv.DeviceArray.from_host(fd)
    for radius in (np.float32(4) * dps, np.float32(np.inf)):
        out = mv.DeviceArray(2048, np.uint16)
        svo.surface_ao_device(2048, dfv, dfd, 16, radius, out)
        want = expected_open(t, radius)
        assert np.array_equal(out.to_host(), want), radius
        assert (want < 16).sum() >= 200 and (want == 16).sum() >= 200  # occluded and open faces both
