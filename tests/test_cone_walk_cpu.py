"""The cone-limited walk of include/mvrt/device.hpp (mvrt::DeviceOctree::intersectCone / intersectConeEx: mvrt_trace_batch_cone, mvrt_render_primary_lod, every
user kernel) without a GPU.  tests/cpp/cone_walk_host.cpp includes the header as it lies behind the stand-in hip_runtime.h and is built twice as a stand-alone
program, as tests/test_lane_walk_cpu.py builds its own: with g++ -O2 -ffp-contract=off, and with -fsanitize=address,undefined.  Both run as subprocesses on files;
nothing is loaded into this process.

The yardstick is the scalar model of tests/lod_expected.py on a pointer-free octree.  It is validated first: with the cone off it equals the oracle's Scene.trace
in t, nMajor and descents on every ray of every scene, bit for bit.  Then the header equals the model in t, nMajor, level, cellCode and descents on every ray, in
both flavours and both stack modes, on the bunny at 2^3 .. 64^3, the three hand-made sets and the 16-level scene of tests/lane_walk_expected.py, with coneA and
coneB cycling over {0, 2^-9, 2^-5, +inf, -1, NaN}^2 and the fixed depths.  The consequences of the rule that the header states are held on the same rays."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import lane_walk_expected as E
import lod_expected as L
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GXX = shutil.which("g++")
COMMON = ["-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "tests", "cpp", "hip_host"), "-I", os.path.join(ROOT, "include")]
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
ALL_SCENES = L.SCENES + (L.DEEP,)

pytestmark = pytest.mark.skipif(GXX is None, reason="no g++")


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("cone_walk")
    out = {}
    for name, flags in BUILDS.items():
        out[name] = str(d / ("cone_walk_host_" + name))
        r = subprocess.run([GXX] + COMMON + flags + [L.CONE_WALK_SRC, "-o", out[name]], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stderr  # (warning-free, too)
    return out


def view_bytes(s):
    import massivevoxelraytracing_amd as mv
    nodes = s.sc.nodes
    v = mv.DeviceOctree()
    v.structBytes, v.flavour = 128, 0 if s.embedded else 1
    v.lower[:], v.upper[:] = s.lower.tolist(), s.upper.tolist()
    v.dps, v.emissionScale, v.hasEmission = s.sc.dps, 1.0, 1
    v.levels, v.numberOfNodes, v.numberOfVoxels = s.levels, len(nodes), len(s.codes)
    v.rootIndex, v.rootMask = len(nodes) - 1, int(nodes["mask"][-1])
    return bytes(v)


def run(program, tmp_path, s, stack_mode, cone_a=None, cone_b=None):
    """-> (intersectConeEx, intersectCone, the bytes of the output file)"""
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    lines, masks, cold = E.node_lines(s.sc.nodes, s.embedded)
    n = L.write_input(src, view_bytes(s), lines, masks, cold, stack_mode, s.ro, s.rd, s.cone_a if cone_a is None else cone_a, s.cone_b if cone_b is None else cone_b)
    r = subprocess.run([program, src, dst], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-4000:])
    ex, plain = L.read_output(dst, n)
    with open(dst, "rb") as f:
        return ex, plain, f.read()


def same(got, want, keys, what):
    for k in keys:
        eq = L.bits(got[k]) == L.bits(want[k])
        assert eq.all(), "%s: %s differs on %d of %d rays, first at %d" % (what, k, (~eq).sum(), eq.size, np.argmax(~eq))


@pytest.mark.parametrize("scene", ALL_SCENES)
def test_model_with_the_cone_off_is_the_oracle(scene):
    s = L.scene(O, scene)
    hits = s.validate()
    assert len(s.ro) <= L.N_RAYS and hits >= len(s.ro) // 4
    if scene != L.DEEP:
        big = np.abs(s.ro[s.outside] - (s.lower + s.upper) / 2).max(1)
        assert (big >= np.float32(0.74) * (s.upper - s.lower).max()).all()  # outside by a quarter extent
        assert ((s.rd[s.outside] == 0).sum(1) == 1).sum() >= 100 and ((s.rd[s.outside] == 0).sum(1) == 2).sum() >= 100
        assert ((s.rd[~s.outside] == 0).any(1)).sum() >= 100


@pytest.mark.parametrize("embedded", [True, False], ids=["embedded", "plain"])
@pytest.mark.parametrize("scene", ALL_SCENES)
def test_host_walk_equals_the_model(programs, tmp_path, scene, embedded):
    s = L.scene(O, scene, embedded)
    s.validate()
    for stack_mode in (0, 1):
        ex, plain, _ = run(programs["plain"], tmp_path, s, stack_mode)
        same(ex, s.on, L.OUTPUTS, "%s stack mode %d" % (scene, stack_mode))
        same(plain, s.on, L.OUTPUTS[:4], "%s stack mode %d, intersectCone" % (scene, stack_mode))
    on, off = s.on, s.off
    hit_on, hit_off = on["t"] != L.MAXF, off["t"] != L.MAXF
    # what the header states of the rule
    assert (on["descents"] <= off["descents"]).all()
    assert hit_on[hit_off].all()
    with np.errstate(invalid="ignore"):
        no_cone = ~((s.cone_a > 0) | (s.cone_b > 0))  # zero, negative and NaN in both: never a footprint above 0
    assert no_cone.sum() >= len(s.ro) // 8
    same({k: on[k][no_cone] for k in L.OUTPUTS}, {k: off[k][no_cone] for k in L.OUTPUTS}, ("t", "nMajor", "descents"), scene + ", no cone")
    assert (on["level"][~hit_on] == 0).all() and (on["cellCode"][~hit_on] == 0).all() and (on["nMajor"][~hit_on] == -1).all()
    stopped = hit_on & (on["level"] < s.levels)
    if s.levels > 1:
        assert stopped.sum() >= 100 and (on["level"][stopped] >= 1).all()
        assert len(set(on["level"][stopped].tolist())) == s.levels - 1  # every inner level stops some ray
        # a stopped ray names a cell that holds voxels
        for lv in set(on["level"][stopped].tolist()):
            sel = stopped & (on["level"] == lv)
            assert np.isin(on["cellCode"][sel], s.codes >> np.uint64(3 * (s.levels - lv))).all()
        if scene != L.DEEP:
            inf = np.isinf(s.cone_a) & (s.cone_a > 0) & (s.cone_b == 0) & s.outside & hit_on
            assert (on["level"][inf] == 1).all() and inf.sum() >= 10  # +inf stops at level 1: from outside every node is entered in front of the origin
    else:
        assert not stopped.any()  # one level: no inner level, the cone changes nothing
        same(on, off, L.OUTPUTS, scene)
    if scene == "between":
        assert (hit_on & ~hit_off).sum() >= 10  # the ray passes between the voxels of one coarse cell: the cone hits, the unlimited ray misses
    print("%s %s: %d rays, %d hits without the cone, %d with it (%d stopped above the voxels, levels %s), descents %d -> %d" % (
        scene, "embedded" if embedded else "plain", len(s.ro), hit_off.sum(), hit_on.sum(), stopped.sum(), np.bincount(on["level"], minlength=s.levels + 1).tolist(),
        off["descents"].sum(), on["descents"].sum()))


@pytest.mark.parametrize("stack_mode", [0, 1], ids=["own_stack", "callers_stack"])
@pytest.mark.parametrize("embedded", [True, False], ids=["embedded", "plain"])
def test_sanitized_walk_at_16_levels(programs, tmp_path, embedded, stack_mode):
    """address and undefined-behaviour sanitizers on the 16-level scene: exit status 0, nothing on stderr, and the bytes of the plain build"""
    s = L.scene(O, L.DEEP, embedded)
    assert s.levels == 16
    ex, plain, raw = run(programs["sanitized"], tmp_path, s, stack_mode)
    same(ex, s.on, L.OUTPUTS, "sanitized")
    same(plain, s.on, L.OUTPUTS[:4], "sanitized, intersectCone")
    assert raw == run(programs["plain"], tmp_path, s, stack_mode)[2]


def test_sanitized_walk_of_the_small_scenes(programs, tmp_path):
    for scene in ("bunny2", "bunny8", "twins"):
        s = L.scene(O, scene)
        ex, _, _ = run(programs["sanitized"], tmp_path, s, 1)
        same(ex, s.on, L.OUTPUTS, scene + ", sanitized")


def test_twins_share_their_nodes_and_not_their_colours():
    """the hand-made set whose two blocks are one DAG node: a colour per node cannot tell them apart, the pyramid keyed by the cell's code does"""
    s = L.scene(O, "twins")
    nodes = s.sc.nodes
    last = nodes["children"][-1][nodes["children"][-1] != 0xFFFFFFFF] & 0xFFFFFF  # the root's children
    below = [set((nodes["children"][k][nodes["children"][k] != 0xFFFFFFFF] & 0xFFFFFF).tolist()) for k in last]
    assert len(below) == 2 and below[0] == below[1]  # both 4^3 cells lead to the same 2^3 node
    lv = s.level(2)
    assert len(lv["code"]) == 2 and lv["count"].tolist() == [4, 4]
    assert lv["attribs"][0, :3].tolist() == [200, 40, 10] and lv["attribs"][1, :3].tolist() == [10, 60, 220]


def test_interface_is_declared_in_every_layer():
    import massivevoxelraytracing_amd as mv
    header = open(os.path.join(ROOT, "include", "mvrt.h")).read()
    mirror = open(os.path.join(ROOT, "include", "mvrt", "IntersectorOctreeGPU.hpp")).read()
    device = open(os.path.join(ROOT, "include", "mvrt", "device.hpp")).read()
    for name in ("mvrt_trace_batch_cone", "mvrt_render_primary_lod", "mvrt_svo_lod_prepare", "mvrt_svo_lod_release", "mvrt_svo_lod_bytes", "mvrt_svo_lod_view"):
        assert name + "(" in header and name in mv.SIGNATURES and name + "(" in mirror
    for name in ("lod_prepare", "lod_release", "lod_view", "lod_bytes", "intersect_cone", "intersect_cone_device", "render_lod"):
        assert callable(getattr(mv.IntersectorOctreeGPU, name))
    for name in ("intersectCone(", "intersectConeEx(", "template <bool RANGE, bool CONE>", "struct DeviceLod", "lookup("):
        assert name in device
    import ctypes
    assert ctypes.sizeof(mv.DeviceLod) == 488 and mv.DeviceLod.codes.offset == 8 and mv.DeviceLod.attrs.offset == 144 and mv.DeviceLod.cellVoxels.offset == 280
    assert mv.DeviceLod.count.offset == 416
    lib = mv.lib()  # the refusals the arguments alone decide, without a GPU call
    p = ctypes.addressof(ctypes.create_string_buffer(64))
    assert lib.mvrt_trace_batch_cone(None, 1, p, p, p, p, p, p, None, p, p, None, None, None, None, None, None, None) != 0 and b"coneADev" in lib.mvrt_last_error()
    assert lib.mvrt_trace_batch_cone(None, 1, p, p, p, p, p, p, p, p, None, None, None, None, None, None, None, None) != 0 and b"t output" in lib.mvrt_last_error()
    assert lib.mvrt_trace_batch_cone(None, 1, p, None, p, p, p, p, p, p, p, None, None, None, None, None, None, None) != 0 and b"null ray array" in lib.mvrt_last_error()
    assert lib.mvrt_trace_batch_cone(None, 1, p, p, p, p, p, p, p, p, p, None, None, None, None, None, None, None) != 0 and b"no octree" in lib.mvrt_last_error()
    assert lib.mvrt_svo_lod_prepare(None, None) != 0 and b"null handle" in lib.mvrt_last_error()
    assert lib.mvrt_svo_lod_bytes(None) == 0
