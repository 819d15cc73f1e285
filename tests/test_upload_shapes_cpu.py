"""The upload contract without a GPU (include/mvrt.h, mvrt_svo_check_upload): the generators of tests/upload_shapes.py keep the geometry the oracle
traces, the library's checker accepts every legal shape and every octree the GPU suite uploads, agrees with the plain-Python model on a seeded fuzz
of single mutations, and mvrt_svo_upload rejects malformed arrays with the checker's message before any HIP call."""
import ctypes as C
import os
import re
from collections import Counter

import numpy as np
import pytest

import deep_scenes as D
import upload_shapes as U
from common import bunny_tris, position_colors
from fixtures import bunny256, O  # noqa: F401 (fixtures)
from rays import random_rays

import massivevoxelraytracing_amd as mv

check = mv.IntersectorOctreeGPU.check_upload


def verdict(msg):
    """checker text -> (accepted, rule, node)"""
    if msg is None:
        return True, None, None
    r = re.search(r"rule (\d)", msg)
    n = re.search(r": node (\d+)", msg)
    return False, int(r.group(1)) if r else None, int(n.group(1)) if n else None


def legal_shapes(t, rng):
    """{name: octree} of the legal generators applied to octree t (and a few compositions)"""
    nodes, nv, res, emb = t
    out = {
        "builder": t,
        "permute": (U.permute(nodes, emb, rng), nv, res, emb),
        "unreachable": (U.add_unreachable(nodes, emb, rng), nv, res, emb),
        "unshare": (U.unshare(nodes, emb), nv, res, emb),
        "empty_inner": (U.add_empty_inner(nodes, res, emb, rng), nv, res, emb),
        "psum_zero": (U.psum_zero(nodes), nv, res, emb),
        "psum_random": (U.psum_random(nodes, nv, res, rng), nv, res, emb),
    }
    out["all"] = (U.permute(U.add_unreachable(U.add_empty_inner(U.unshare(nodes, emb), res, emb, rng), emb, rng), emb, rng), nv, res, emb)
    if ((nodes["children"] == U.LEAF) & ((nodes["mask"][:, None] >> np.arange(8)) & 1).astype(bool)).sum(1).max() >= 2:
        out["psum_one_off"] = (U.psum_one_off(nodes, emb, rng)[0], nv, res, emb)
    return out


# ---- the generators keep the geometry ----------------------------------------------------------------------------------------------------------
def trace(O, sc, nodes, emb, ro, rd, sh):
    return O.Scene(nodes, sc.attrs, sc.origin, sc.dps, sc.grid_res, sc.has_emission, embedded=emb).trace(ro, rd, sh, threads=8, want_descents=True)


@pytest.mark.parametrize("emb", [True, False])
@pytest.mark.parametrize("scene", ["bunny256", "random7"])
def test_generated_shapes_trace_like_the_builder_octree(O, bunny256, scene, emb):
    """permuted, padded with unreachable nodes and unshared octrees give the oracle's t, nMajor, vIndex and descents of the builder's octree of the
    same voxels; reachable empty nodes keep t, nMajor and vIndex, and descents only grow"""
    rng = np.random.default_rng(11 if emb else 12)
    if scene == "bunny256":
        sc = bunny256 if emb else O.build_scene_from_triangles(bunny_tris(), 256, embed=False)
    else:
        codes = np.unique(rng.integers(0, 1 << 21, 3000, dtype=np.uint64))
        attrs = rng.integers(0, 256, (len(codes), 8), dtype=np.uint8)
        sc = O.Scene(O.build_octree(codes, 128, embed=emb), attrs, (0.0, 0.0, 0.0), 1.0 / 128, 128, 1, embedded=emb)
    ro, rd = random_rays(sc, 30_000, 5)
    sh = (np.arange(len(ro)) % 4 == 0).astype(np.uint8)
    want = trace(O, sc, sc.nodes, emb, ro, rd, sh)
    assert (want["t"] != O.MAX_FLOAT).sum() > 2000
    for name, nodes in (("permute", U.permute(sc.nodes, emb, rng)), ("unreachable", U.add_unreachable(sc.nodes, emb, rng, 20, 20)),
                        ("unshare", U.unshare(sc.nodes, emb)), ("unshare+permute", U.permute(U.unshare(sc.nodes, emb), emb, rng))):
        assert check(nodes, len(sc.attrs), sc.grid_res, emb) is None, name
        got = trace(O, sc, nodes, emb, ro, rd, sh)
        for k in ("t", "nMajor", "vIndex", "descents"):
            assert np.array_equal(got[k], want[k]), (name, k)
    empty = U.add_empty_inner(U.permute(sc.nodes, emb, rng), sc.grid_res, emb, rng, count=200)
    assert check(empty, len(sc.attrs), sc.grid_res, emb) is None
    assert (empty["mask"] == 0).sum() >= 150
    got = trace(O, sc, empty, emb, ro, rd, sh)
    for k in ("t", "nMajor", "vIndex"):
        assert np.array_equal(got[k], want[k]), k
    assert (got["descents"] >= want["descents"]).all() and (got["descents"] > want["descents"]).sum() > 100


# ---- the checker accepts what it must ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", range(1, 22))
def test_checker_accepts_builder_octrees_at_every_depth(O, levels):
    rng = np.random.default_rng(levels)
    for dag in (True, False):
        for emb in (True, False):
            t = U.small_octree(O, rng, levels, dag, emb, n_voxels=int(rng.integers(1, 300)))
            assert check(*t) is None, (levels, dag, emb, check(*t))
            assert U.check_model(*t) == (True, None, None)
            assert len(U.voxel_paths(t[0], t[2], emb)) == t[1]


def test_checker_accepts_every_legal_generated_shape(O):
    rng = np.random.default_rng(3)
    seen = Counter()
    for levels in range(1, 7):
        for dag in (True, False):
            for emb in (True, False):
                for _ in range(4):
                    t = U.small_octree(O, rng, levels, dag, emb)
                    for name, s in legal_shapes(t, rng).items():
                        assert check(*s) is None, (name, levels, dag, emb, check(*s))
                        assert U.check_model(*s) == (True, None, None), name
                        seen[name] += 1
    # the empty octree, in both flavours, and voxels without attributes are not needed by an empty one
    empty = np.zeros(1, O.NODE_DTYPE)
    empty["children"] = U.LEAF
    for emb in (True, False):
        for res in (2, 256, 1 << 21):
            assert check(empty, 0, res, emb) is None and U.check_model(empty, 0, res, emb)[0]
    print("legal shapes checked:", dict(seen))


def test_checker_accepts_every_octree_the_gpu_suite_uploads(O, bunny256):
    """bunny 256 (DAG and plain tree), its all-0 and all-3 nVoxelsPSum variants, the triangle scenes of the path-tracer tests and the deep_scenes
    octrees of 14-21 levels, rebuilt here with the seeds the GPU tests use: the new rules break no existing test"""
    n = len(bunny256.attrs)
    assert check(bunny256.nodes, n, 256, True) is None
    plain = O.build_octree(bunny256.morton, 256, dag=False, embed=False)
    assert check(plain, n, 256, False) is None
    assert check(O.build_octree(bunny256.morton, 256, dag=True, embed=False), n, 256, False) is None
    for v in (0, 3):
        nodes = bunny256.nodes.copy()
        nodes["psum"][:] = v
        assert check(nodes, n, 256, True) is None
    tris = bunny_tris()
    cols, emis = position_colors(tris)
    for res in (2, 4, 8, 16, 64, 128):
        for dag, emb in ((True, True), (False, False)):
            sc = O.build_scene_from_triangles(tris, res, cols, emis, dag=dag, embed=emb)
            assert check(sc.nodes, len(sc.attrs), res, emb) is None, res
    for levels in D.DEPTHS:
        for seed in (None, 50 + levels):
            s = D.DeepScene(levels, seed=seed)
            if seed is not None:  # test_cell_index_boundary's extra voxels
                rng = np.random.default_rng(levels)
                s.xyz = np.concatenate([s.xyz, rng.integers(0, s.res, size=(40_000, 3)).astype(np.uint32)])
                s.attrs = np.concatenate([s.attrs, rng.integers(0, 256, size=(40_000, 8)).astype(np.uint8)])
                s.morton = np.unique(D.morton(s.xyz))
            sc = D.oracle_scene(O, s)
            assert check(sc.nodes, len(sc.attrs), s.res, True) is None, levels


# ---- checker == model on single mutations ------------------------------------------------------------------------------------------------------
def test_named_mutations_break_their_rule(O):
    rng = np.random.default_rng(17)
    hits = Counter()
    for levels in range(1, 7):
        for dag in (True, False):
            for emb in (True, False):
                t = U.small_octree(O, rng, levels, dag, emb, n_voxels=int(rng.integers(2, 60)))
                for name, mut in U.MUTATIONS.items():
                    m = mut(t, rng)
                    if m is None:
                        continue
                    *bad, rule = m
                    want = U.check_model(*bad)
                    assert want[0] is False and want[1] == rule, (name, levels, dag, emb, want)
                    assert verdict(check(*bad)) == want, (name, levels, dag, emb, check(*bad), want)
                    hits[name] += 1
    print("named mutations:", dict(hits))
    assert set(hits) == set(U.MUTATIONS)
    msg = check(*U.mut_coarse_voxel(U.small_octree(O, rng, 4, True, True, 30), rng)[:4])
    assert "voxels above the last level (coarse voxels) are not supported" in msg


def test_fuzz_checker_agrees_with_the_model(O):
    """a seeded fuzz of single random mutations of small octrees (1-6 levels, DAG and tree, both flavours, legal shapes first): the checker's
    verdict, rule and first offending node equal the model's on every case"""
    rng = np.random.default_rng(2026)
    per_rule = Counter()
    names = list(U.MUTATIONS) + ["random_word"] * 6
    n_cases = 3000
    for i in range(n_cases):
        t = U.small_octree(O, rng, int(rng.integers(1, 7)), bool(rng.integers(0, 2)), bool(rng.integers(0, 2)))
        shapes = legal_shapes(t, rng)
        base = shapes[list(shapes)[int(rng.integers(0, len(shapes)))]]
        name = names[int(rng.integers(0, len(names)))]
        m = (U.mut_random_word if name == "random_word" else U.MUTATIONS[name])(base, rng)
        if m is None:
            m = U.mut_random_word(base, rng)
        bad = m[:4]
        want = U.check_model(*bad)
        got = verdict(check(*bad))
        assert got == want, (i, name, got, want, check(*bad))
        per_rule["accepted" if want[0] else "rule %d" % want[1]] += 1
    print("fuzz: %d mutations, verdicts per rule: %s" % (n_cases, dict(sorted(per_rule.items()))))
    for k in ("accepted", "rule 1", "rule 2", "rule 3", "rule 4"):
        assert per_rule[k] >= 100, (k, per_rule)


def test_rule_1_answers_every_int32_grid_res(O):
    """gridRes is checked for range and power of two before anything is derived from it: values above 2^30 once made the log2 loop run
    forever.  Each value goes through the checker, the upload and the three build entry points in a child process with a time limit."""
    import subprocess
    import sys
    code = """
import ctypes as C, sys
import numpy as np
sys.path.insert(0, %r)
import massivevoxelraytracing_amd as mv
lib = mv.lib()
root = np.zeros(68, np.uint8)
root.view(np.uint32)[1:9] = 0xFFFFFFFF
rp = root.ctypes.data_as(C.c_void_p)
h = C.c_void_p(0)
assert lib.mvrt_svo_create(C.byref(h)) == 0
o = np.zeros(3, np.float32)
op = o.ctypes.data_as(C.c_void_p)
v = np.zeros(9, np.float32)
for res in %r:
    assert lib.mvrt_svo_check_upload(rp, 1, 0, res, 1) != 0 and b"rule 1" in lib.mvrt_last_error(), res
    assert lib.mvrt_svo_upload(h, rp, 1, None, 0, op, 0.1, res, 0, 1, None) != 0 and b"rule 1" in lib.mvrt_last_error(), res
    assert lib.mvrt_svo_build_voxels(h, 0x1000, None, 8, op, 0.1, res, 0, None) != 0 and b"gridRes" in lib.mvrt_last_error(), res
    assert lib.mvrt_svo_build_synthetic(h, res, 8, 1, op, 0.1, 0, None) != 0 and b"gridRes" in lib.mvrt_last_error(), res
    if res < 2 or res & (res - 1):  # (powers of two above 2^21 are legal for triangle builds)
        assert lib.mvrt_svo_build_ex(h, v.ctypes.data_as(C.c_void_p), None, None, 3, None, op, 0.1, res, 0) != 0 and b"gridRes" in lib.mvrt_last_error(), res
print("ok", len(%r))
""" % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), U.GARBAGE_GRID_RES, U.GARBAGE_GRID_RES)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stderr[-2000:]
    one = np.zeros(1, O.NODE_DTYPE)
    one["children"] = U.LEAF
    for res in U.GARBAGE_GRID_RES:
        assert U.check_model(one, 0, res, True) == (False, 1, None)
        assert verdict(check(one, 0, res, True)) == (False, 1, None), res


def test_rule_5_and_the_numbering_limit():
    one = np.zeros(68, np.uint8)
    lib = mv.lib()
    # rule 5 is decided from the count alone, before any node is read
    assert lib.mvrt_svo_check_upload(one.ctypes.data_as(C.c_void_p), 0xFFFFFF, 1, 256, 1) != 0
    assert "rule 5" in lib.mvrt_last_error().decode()
    assert lib.mvrt_svo_check_upload(None, 0, 0, 256, 1) != 0 and "empty octree" in lib.mvrt_last_error().decode()


# ---- mvrt_svo_upload rejects on the host -------------------------------------------------------------------------------------------------------
def test_upload_rejects_malformed_arrays_before_any_hip_call(O):
    lib = mv.lib()
    h = C.c_void_p(0)
    assert lib.mvrt_svo_create(C.byref(h)) == 0  # host allocation only
    try:
        rng = np.random.default_rng(5)
        t = U.small_octree(O, rng, 4, True, True, 50)
        o = np.zeros(3, np.float32)
        attrs = np.zeros((max(t[1], 1), 8), np.uint8)
        cases = [U.MUTATIONS[k](t, rng)[:4] for k in ("child_out_of_range", "garbage_in_absent_slot", "wrong_embedded_byte", "plain_indices_as_embedded",
                                                       "self_loop", "coarse_voxel", "grid_halved", "grid_doubled", "grid_2_22", "node_at_two_depths",
                                                       "psum_reaches_count", "voxels_without_count")]
        for nodes, nv, res, emb in cases:
            want = check(nodes, nv, res, emb)
            assert want is not None
            rc = lib.mvrt_svo_upload(h.value, nodes.ctypes.data_as(C.c_void_p), len(nodes), attrs.ctypes.data_as(C.c_void_p), nv, o.ctypes.data_as(C.c_void_p),
                                     1.0 / 16, res, 0, int(emb), None)
            assert rc != 0 and lib.mvrt_last_error().decode() == want
            i = mv.SvoInfo()
            assert lib.mvrt_svo_get_info(h.value, C.byref(i)) == 0
            assert (i.numberOfNodes, i.numberOfVoxels, i.gridRes) == (0, 0, 0)
    finally:
        lib.mvrt_svo_destroy(h.value)


def test_header_and_mirrors_declare_the_checker():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "int mvrt_svo_check_upload(" in open(os.path.join(root, "include", "mvrt.h")).read()
    assert "mvrt_svo_check_upload" in mv.SIGNATURES
    assert "checkUpload(" in open(os.path.join(root, "include", "mvrt", "IntersectorOctreeGPU.hpp")).read()
