"""The per-lane octree walk of include/mvrt/device.hpp (mvrt::DeviceOctree::walk<RANGE>: every user kernel, mvrt_trace_batch_range, occluded(), the occlusion
bake) without a GPU.  tests/cpp/lane_walk_host.cpp includes the header as it lies behind a stand-in hip_runtime.h and is built twice as a stand-alone program: with
g++ -O2 -ffp-contract=off, and with -fsanitize=address,undefined.  Both run as subprocesses on files; nothing is loaded into this process.

Against the oracle, bit for bit (tests/lane_walk_expected.py has the rays and the expectations): bunny64, random9, deep14 and deep16 -- 16 levels, the deepest the
device view accepts --, embedded and plain, on R.rays_of plus 160 000 far-origin rays; unlimited (t, nMajor, vIndex, descents) and under the limit cycle of
tests/test_gpu_range.py (the filtered oracle, descents, occluded).  The sanitized build walks deep16 in both flavours and both stack modes: the 3-bits-per-level
registers (resume, path, pending) are shifted at the level limit by rays that pop from the last level to the root, the caller's stack holds exactly `levels` entries.

What a wrong early-exit margin does here (tried on a scratch copy, margin factor 16 -> 0): the limited t differs from the filtered oracle on 3 131 (deep16) to
3 994 (bunny64) rays of the limit cases `t` and `above`, on every scene and flavour -- hits within the limit that the cut dropped.  `S <= tMax` -> `S < tMax` fails the
same comparison on every hit of the case `t`.  A caller's stack one entry short fails the sanitized run alone (heap-buffer-overflow)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import lane_walk_expected as E
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GXX = shutil.which("g++")
COMMON = ["-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "tests", "cpp", "hip_host"), "-I", os.path.join(ROOT, "include")]
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}

pytestmark = pytest.mark.skipif(GXX is None, reason="no g++")


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("lane_walk")
    out = {}
    for name, flags in BUILDS.items():
        out[name] = str(d / ("lane_walk_host_" + name))
        r = subprocess.run([GXX] + COMMON + flags + [E.LANE_WALK_SRC, "-o", out[name]], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stderr  # (warning-free, too)
    return out


def run(program, tmp_path, exp, stack_mode, rays=None):
    """-> (unlimited, limited, the bytes of the output file)"""
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    n = E.write_input(src, exp, stack_mode, rays=rays)
    r = subprocess.run([program, src, dst], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-4000:])
    unlimited, limited = E.read_output(dst, n)
    with open(dst, "rb") as f:
        return unlimited, limited, f.read()


@pytest.mark.parametrize("embedded", [True, False], ids=["embedded", "plain"])
@pytest.mark.parametrize("scene", E.SCENES)
def test_host_walk_equals_the_oracle(programs, tmp_path, scene, embedded):
    exp = E.expectation(O, scene, embedded)
    per_k = exp.check_populations()
    assert np.isnan(exp.rd).any() and np.isinf(exp.rd).any() and exp.n_base - exp.n_set == E.N_FAR
    unlimited, limited, _ = run(programs["plain"], tmp_path, exp, 1)
    exp.check_unlimited(unlimited, "caller's stack")
    exp.check_limited(limited, "caller's stack")
    far = exp.far_k >= 0
    full, de = exp.want["descents"], limited["descents"]
    quarter = exp.case == E.CASES.index("quarter")
    assert de[quarter].sum(dtype=np.uint64) < full[quarter].sum(dtype=np.uint64)  # there is a cut at all
    walked = exp.case < E.CASES.index("zero")  # the limits above 0: the others return before the walk
    cut = walked & (de < full)
    print("%s %s: %d rays, %d hits (%d at t = +inf), far hits per k %s; of %d rays with a limit above 0 (%d far) the cut ended %d (%d far) early and saved %d descents (%d on far rays)" % (
        scene, "embedded" if embedded else "plain", len(exp.ro), (exp.want["t"] != E.MAXF).sum(), exp.n_inf, per_k.tolist(), walked.sum(), (walked & far).sum(), cut.sum(),
        (cut & far).sum(), int(full[walked].sum(dtype=np.uint64) - de[walked].sum(dtype=np.uint64)), int(full[walked & far].sum(dtype=np.uint64) - de[walked & far].sum(dtype=np.uint64))))


@pytest.mark.parametrize("stack_mode", [0, 1], ids=["own_stack", "callers_stack"])
@pytest.mark.parametrize("embedded", [True, False], ids=["embedded", "plain"])
def test_sanitized_walk_at_16_levels(programs, tmp_path, embedded, stack_mode):
    """address and undefined-behaviour sanitizers on the whole input of deep16: exit status 0, nothing on stderr, and the bytes of the plain build"""
    exp = E.expectation(O, "deep16", embedded)
    assert exp.rs.levels == 16
    # rays that pop from the last level towards the root: the walk went below level 15 and yet made more descents than one path holds
    deep = (exp.want["descents"] > 2 * 16) & (exp.want["t"] != E.MAXF)
    assert deep.sum() >= 1000
    unlimited, limited, raw = run(programs["sanitized"], tmp_path, exp, stack_mode)
    exp.check_unlimited(unlimited, "sanitized")
    exp.check_limited(limited, "sanitized")
    assert raw == run(programs["plain"], tmp_path, exp, stack_mode)[2]


def test_node_lines_of_the_plain_flavour():
    """the layout this file hands to the walk, on a hand-made octree: child masks per byte, 0 for voxels and absent children"""
    nodes = np.zeros(3, O.NODE_DTYPE)
    nodes["children"][:] = 0xFFFFFFFF
    nodes["mask"] = [0x81, 0x18, 0x06]
    nodes["children"][2, 1], nodes["children"][2, 2] = 0, 1
    nodes["psum"][2] = np.arange(8)
    lines, masks, cold = E.node_lines(nodes, False)
    assert lines[2, 8] == (0x81 << 8) | (0x18 << 16) and lines[2, 9] == 0 and (lines[:2, 8:] == 0).all() and (lines[:, 10:] == 0).all()
    assert masks.tolist() == [0x81, 0x18, 0x06] and cold[2].tolist() == list(range(8))
    emb, m, c = E.node_lines(nodes, True)
    assert m is None and c is None and emb[2, 8:].tolist() == list(range(8)) and np.array_equal(emb[:, :8], nodes["children"])
