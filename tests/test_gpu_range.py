"""Distance-limited rays on the MI355X: mvrt_trace_batch_range and a user kernel on the limited methods of include/mvrt/device.hpp (tests/hip/range_probe.hip,
both stack modes) report, bit for bit, the CPU oracle's unlimited hit where its t <= tMax and a miss otherwise -- on the ray set of tests/rays.py (random,
zero-component, from-inside and dyadic tie rays, 30 % shadow) with a per-ray limit that cycles over t, its two neighbours, 0.25 t, 4 t, MAX_FLOAT, +inf, 0, -1, NaN."""

import numpy as np
import pytest

from common import bunny_tris
from fixtures import mv, O  # noqa: F401 (fixtures)
from lane_walk_expected import CASES, expected, limits  # shared with tests/test_lane_walk_cpu.py and tests/test_gpu_lane_walk_edges.py
from rays import compile_range_probe, probe_range, ray_set, upload

pytestmark = pytest.mark.gpu

MAXF = np.float32(3.402823466e38)
OUTPUTS = ("t", "nMajor", "vIndex", "descents")


@pytest.fixture(scope="module")
def probe(mv, tmp_path_factory):
    return compile_range_probe(tmp_path_factory.mktemp("range_probe"), [])


class Reference:
    """rays, limits and the filtered oracle of one oracle scene: computed once, shared by the tests of that scene, never modified"""

    def __init__(self, sc, n, seed):
        self.sc = sc
        self.ro, self.rd, self.sh = ray_set(sc, n, seed)
        self.want = sc.trace(self.ro, self.rd, self.sh, threads=8, want_descents=True)
        self.tmax, self.case = limits(sc, self.want["t"])
        self.exp, self.keep = expected(self.want, self.sh, self.tmax)
        for a in (self.ro, self.rd, self.sh, self.tmax, self.case, self.keep, *self.want.values(), *self.exp.values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)

    def hits_in(self, name):
        return int(((self.want["t"] != MAXF) & (self.case == CASES.index(name))).sum())


def check(mv, probe, svo, ref, min_case_hits=1000):
    # the two cases a non-conservative cut gets wrong must be well populated
    assert ref.hits_in("t") >= min_case_hits and ref.hits_in("below") >= min_case_hits
    hit = ref.want["t"] != MAXF
    assert ref.keep[hit & (ref.case == CASES.index("t"))].all() and not ref.keep[ref.case == CASES.index("below")].any()
    unlimited = svo.intersect(ref.ro, ref.rd, ref.sh, want_descents=True)
    assert np.array_equal(unlimited["descents"], ref.want["descents"])
    got = [svo.intersect_range(ref.ro, ref.rd, ref.tmax, ref.sh, want_descents=True)]
    view = svo.device_view()
    got += [probe_range(mv, probe, view, ref.ro, ref.rd, ref.sh, ref.tmax, mode) for mode in (0, 1)]
    for g in got:
        for k in ("t", "nMajor", "vIndex"):
            assert np.array_equal(g[k].view(np.uint32), ref.exp[k].view(np.uint32)), k
        de = g["descents"]
        assert np.array_equal(de[ref.keep], unlimited["descents"][ref.keep])  # an accepted hit walked exactly the unlimited walk
        assert (de <= unlimited["descents"]).all()
        quarter = ref.case == CASES.index("quarter")
        assert de[quarter].sum(dtype=np.uint64) < unlimited["descents"][quarter].sum(dtype=np.uint64)  # there is a cut at all
        for name in ("zero", "minus", "nan"):
            assert (de[ref.case == CASES.index(name)] == 0).all()
    for g in got[1:]:
        # occluded() = the limited SHADOW ray of the same origin, direction and limit, whatever the ray's own flag
        assert np.array_equal(g["occluded"], ref.keep.astype(np.uint8))
    assert np.array_equal(got[0]["descents"], got[1]["descents"]) and np.array_equal(got[1]["descents"], got[2]["descents"])


@pytest.fixture(scope="module")
def bunny256(O):
    return {True: O.build_scene_from_triangles(bunny_tris(), 256), False: O.build_scene_from_triangles(bunny_tris(), 256, embed=False)}


@pytest.fixture(scope="module")
def ref256(bunny256):
    return {embed: Reference(sc, 200_000, 7) for embed, sc in bunny256.items()}


@pytest.mark.parametrize("embedded", [True, False])
def test_uploaded_bunny_256(mv, probe, bunny256, ref256, embedded):
    svo = upload(mv, bunny256[embedded], embedded)
    assert svo.device_view().flavour == (0 if embedded else 1)
    check(mv, probe, svo, ref256[embedded])


@pytest.mark.parametrize("flags", [0, 2])
def test_gpu_built_bunny_256(mv, probe, ref256, flags):
    from massivevoxelraytracing_amd import scenes
    v = bunny_tris().reshape(-1, 3)
    origin, dps = scenes.bounding_grid(v, 256)
    svo = mv.IntersectorOctreeGPU()
    svo.build(v, None, None, None, origin, dps, 256, flags=flags)
    assert svo.device_view().flavour == (1 if flags & 2 else 0)
    check(mv, probe, svo, ref256[(flags & 2) == 0])


@pytest.mark.parametrize("res", [2, 4, 8])
def test_tiny_grids(mv, O, probe, res):
    sc = O.build_scene_from_triangles(bunny_tris(), res)
    check(mv, probe, upload(mv, sc), Reference(sc, 20_000, res))


def test_empty_batch(mv, probe, bunny256):
    svo = upload(mv, bunny256[True])
    out = svo.intersect_range(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0), want_descents=True)
    assert all(len(out[k]) == 0 for k in OUTPUTS)
    assert mv.lib().mvrt_trace_batch_range(svo._h, 0, *([None] * 7), 1, 1, None, None, None, None) == 0  # no launch: the pointers are never read


def test_scalar_limit_and_optional_outputs(mv, bunny256, ref256):
    ref = ref256[True]
    svo = upload(mv, bunny256[True])
    n = 20_000
    lim = np.float32(np.median(ref.want["t"][:n][ref.want["t"][:n] != MAXF]))
    want = {k: ref.want[k][:n] for k in OUTPUTS}
    exp, keep = expected(want, ref.sh[:n], lim)
    assert 0 < keep.sum() < (ref.want["t"][:n] != MAXF).sum()
    assert np.array_equal(svo.intersect_range(ref.ro[:n], ref.rd[:n], lim, ref.sh[:n])["t"], exp["t"])
    dev = [mv.DeviceArray.from_host(np.ascontiguousarray(a)) for a in (*ref.ro[:n].T, *ref.rd[:n].T)]
    t = mv.DeviceArray(n, np.float32)
    dlim = mv.DeviceArray.from_host(np.full(n, lim, np.float32))
    svo.intersect_range_device(n, *dev, None, dlim, t)  # t alone, no shadow flags
    mv.synchronize()
    assert np.array_equal(t.to_host(), expected(want, np.zeros(n, np.uint8), lim)[0]["t"])


def test_tree_flavour_is_refused_by_name(mv):
    from massivevoxelraytracing_amd import scenes
    v = bunny_tris().reshape(-1, 3)
    origin, dps = scenes.bounding_grid(v, 128)
    svo = mv.IntersectorOctreeGPU()
    svo.build(v, None, None, None, origin, dps, 128, flags=mv.IntersectorOctreeGPU.BUILD_NO_DAG | mv.IntersectorOctreeGPU.BUILD_NO_EMBEDDED_MASK)
    assert svo.info().flavour == 2
    z = np.zeros((4, 3), np.float32)
    with pytest.raises(mv.MvrtError, match="mvrt_trace_batch_range: tree-flavour"):
        svo.intersect_range(z, z + 1, 1.0)
    one = mv.DeviceArray(1, np.uint32)
    with pytest.raises(mv.MvrtError, match="mvrt_svo_surface_ao: tree-flavour"):
        svo.surface_ao_device(1, one, one, 16, 1.0, one)


def test_contract_on_build_gives_identical_output(mv, probe, bunny256, ref256, tmp_path):
    on = compile_range_probe(tmp_path, ["-ffp-contract=on"])
    ref = ref256[True]
    svo = upload(mv, bunny256[True])  # (kept alive: the view is a snapshot of its buffers)
    view = svo.device_view()
    n = 50_000
    args = (ref.ro[:n], ref.rd[:n], ref.sh[:n], ref.tmax[:n])
    for mode in (0, 1):
        a, b = probe_range(mv, on, view, *args, mode), probe_range(mv, probe, view, *args, mode)
        for k in OUTPUTS + ("occluded",):
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
