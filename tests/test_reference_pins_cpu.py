"""The CPU oracle (oracle/mvrt_oracle.cpp) against the COMPILED reference, bit for bit: the voxelizer's VTContext, buildOctreeDAGReference /
buildOctreeNaive / embedMask, octreeTraverse_EfficientParametric and the small helpers of voxCommon.hpp, built as they lie into
oracle/_ref/libmvrt_ref_walk.so (oracle/ref_shim_walk.cpp; DESIGN.md section 2 has the flags and the stand-in rule).

Every GPU test of this repository is bit-exact against the oracle, and the oracle is a hand-written restatement: a misreading of the reference
shared by the oracle and the kernels would pass everything else.  Where oracle/_ref is absent the oracle must reproduce the SHA-256 of the
reference's answer stored in tests/golden/reference_pin_digests.json (tests/reference_pins.py::check); where the reference tree is present a missing
library or symbol fails.  No tolerance anywhere.

Not pinned here, because the reference offers nothing to compile: the attribute interpolation (closestBarycentricCoordinateOnTriangle sits in
voxKernel.cu), the non-embedded walk (ENABLE_EMBEDED_MASK is hard-wired, voxCommon.hpp:9), the naive builder's nVoxelsPSum (left unwritten,
IntersectorOctree.hpp:182-196)."""
import numpy as np
import pytest

import deep_scenes as D
import reference_pins as R
from common import bunny_tris
from oracle import oracle as O


@pytest.fixture(scope="module")
def walk():
    return R.load_walk(O, tree_decides=True)


# ---- voxelizer -------------------------------------------------------------------------------------------------------------------------------------
def voxelizer_pin(walk, key, tris, origin, dps, res, six):
    """the dumped list in order (duplicates kept) and the per-triangle counts; -> the counts"""
    m, _ = O.voxelize(tris, origin, dps, res, six_separating=six)
    counts = O.voxelize_counts(tris, origin, dps, res, six_separating=six)
    assert int(counts.sum()) == len(m)
    R.check(key, [m, counts], walk, lambda w: list(w.voxelize(tris, origin, dps, res, six_separating=six)))
    return counts


@pytest.mark.parametrize("six", [True, False], ids=["six", "conservative"])
@pytest.mark.parametrize("res", [16, 64, 256])
def test_voxelizer_bunny(walk, res, six):
    tris = bunny_tris()
    v = tris.reshape(-1, 3)
    origin = v.min(0)
    dps = np.float32(np.float32((v.max(0) - origin).max()) / np.float32(res))  # voxRT.cpp:188-196, as O.build_scene_from_triangles
    counts = voxelizer_pin(walk, "vox/bunny%d/%d" % (res, six), tris, origin, dps, res, six)
    if res == 256 and six:
        assert int(counts.sum()) == 185985  # the survey's golden number of dumped voxels


@pytest.mark.parametrize("six", [True, False], ids=["six", "conservative"])
@pytest.mark.parametrize("res", [32, 4, 2048])
@pytest.mark.parametrize("cls", R.CLASSES)
def test_voxelizer_triangle_classes(walk, cls, res, six):
    origin, dps = R.class_grid(res)
    tris = R.triangle_classes(res)[cls]
    assert tris.shape == (300, 9)
    counts = voxelizer_pin(walk, "vox/%s/%d/%d" % (cls, res, six), tris, origin, dps, res, six)
    if cls == "two_equal":
        assert (counts == 0).all()  # a zero normal: kx, ky are NaN, every comparison of the z range fails, in the reference and here
    elif cls != "clipped":
        assert (counts > 0).sum() >= 200  # the class is no list of refusals (slivers and sub-voxel triangles may slip between voxel centres)
    if cls == "clipped":
        assert 0 < (counts == 0).sum() < 300  # some wholly outside, some not


def test_triangle_classes_are_what_they_say():
    for res in (4, 32, 2048):
        origin, dps = R.class_grid(res)
        cl = R.triangle_classes(res)
        vox = {k: (v.reshape(-1, 3, 3).astype(np.float64) - origin) / float(dps) for k, v in cl.items()}
        assert (vox["lattice"] == np.round(vox["lattice"])).all()
        p = vox["in_plane"]
        flat = (p == p[:, :1]).all(1) & (p[:, 0] == np.round(p[:, 0]))  # an axis on which all three vertices share one integer coordinate
        assert flat.any(1).all()
        e = vox["two_equal"]
        assert ((e[:, 0] == e[:, 1]).all(1) | (e[:, 1] == e[:, 2]).all(1) | (e[:, 2] == e[:, 0]).all(1)).all()
        c = vox["clipped"]
        assert ((c < 0) | (c > res)).any() and ((c > 0) & (c < res)).any()
        s = vox["sub_voxel"]
        assert (s.max(1) - s.min(1)).max() < 1.0


# ---- builder ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def builder_scenes():
    return R.builder_scenes(O)


@pytest.mark.parametrize("embed", [True, False], ids=["embedded", "plain"])
@pytest.mark.parametrize("dag", [True, False], ids=["dag", "naive"])
@pytest.mark.parametrize("scene", ["bunny16", "bunny64", "bunny256", "single1", "random7", "random9", "full8"])
def test_builder(walk, builder_scenes, scene, dag, embed):
    """DAG build: mask, children, psum and node count.  Naive build: mask and children only -- buildOctreeNaive never writes the psum of an absent child."""
    m, res = builder_scenes[scene]
    assert (np.diff(m.astype(np.int64)) > 0).all() and int(m[-1]) < res ** 3
    got = O.build_octree(m, res, dag=dag, embed=embed)
    R.check("build/%s/%d/%d" % (scene, dag, embed), R.node_fields(got, psum=dag), walk,
            lambda w: R.node_fields(w.build_octree(m, res, dag=dag, embed=embed), psum=dag))
    if scene == "full8" and dag:
        assert len(got) == 3  # one node per level: every sibling is shared


# ---- traversal -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", R.RAY_SCENES)
def test_traversal(walk, scene):
    """t by its bits, nMajor and vIndex on ALL rays (a miss keeps the presets MAX_FLOAT, -1, 0): >= 100 000 mixed rays, the tie rays, origins on voxel
    corners / edges / faces, secondary-style origins, direction components of +-0, denormals, huge values, +-inf and NaN (whatever the reference's
    comparisons make of a NaN, the oracle makes the same), a third of them shadow rays.  Embedded walk only."""
    rs = R.ray_scene(O, scene)
    ro, rd, sh = R.rays_of(O, scene)
    assert len(ro) >= 100_000 + 9000 + 6000 + 6000 and np.isnan(rd).any() and np.isinf(rd).any()
    got = rs.sc.trace(ro, rd, sh, threads=8)
    hit = got["t"] != R.MAXF
    assert hit.sum() > 2000 and (~hit).sum() > 2000
    assert (got["vIndex"][sh == 1] == 0).all()
    R.check("trace/" + scene, [got["t"], got["nMajor"], got["vIndex"]], walk,
            lambda w: [x for x in w.trace(rs.nodes, rs.lower, rs.upper, ro, rd, sh).values()])


def test_deep_scenes_fit_the_reference_stack():
    """IntersectorOctree::intersect walks with StackElement stack[32] (IntersectorOctree.hpp:250): 14 to 21 levels fit"""
    assert max(D.DEPTHS) <= 32 and list(R.RAY_SCENES[-len(D.DEPTHS):]) == ["deep%d" % L for L in D.DEPTHS]


# ---- helpers ---------------------------------------------------------------------------------------------------------------------------------------
def helper_answers(hit_n, bsearch, sort_bits, hash_combine, sizes):
    rng = np.random.default_rng(31)
    rds = np.concatenate([rng.normal(size=(40, 3)), [[0, 0, 0], [-0.0, 0.0, -0.0], [np.nan, np.inf, -np.inf], [1e-45, -1e-45, 0]]]).astype(np.float32)
    n = np.array([hit_n(major, rd) for rd in rds for major in (0, 1, 2, -1, 3)], np.float32)
    found = []
    for xs in ([], [5], [5, 5], [1, 3], list(range(0, 40, 3)), sorted(rng.integers(0, 100, 100).tolist()), [-7, -7, 0, 2**31 - 1]):
        found += [bsearch(np.array(xs, np.int32), int(x)) for x in [5, 0, -7, 3, 39, 2**31 - 1, -2**31] + rng.integers(0, 120, 30).tolist()]
    sb = [sort_bits(1 << i) for i in range(22)]
    words = rng.integers(0, 2**32, (200, 4), dtype=np.uint64).astype(np.uint32)
    hc = [hash_combine(*(int(x) for x in w[:k])) for w in words for k in (2, 3, 4)]
    s = sizes()
    return [n, np.array(found, np.int32), np.array(sb, np.int32), np.array(hc, np.uint32), np.array([s["OctreeNode"], s["StackElement"], s["OctreeTask"],
                                                                                                   s["VoxelAttirb"]], np.int32)]


def test_helpers(walk):
    """getHitN (all majors, zero / NaN directions), bSearch (empty and one-element arrays, duplicates, the int range's ends), numberOfSortBitsMorton
    for every power of two up to 2^21, hashCombine of 2, 3 and 4 words, struct sizes"""
    got = helper_answers(O.get_hit_n, O.bsearch, lambda r: 3 * (int(r).bit_length() - 1), lambda a, *w: O.murmur(a, list(w)), O.struct_sizes)
    assert got[2].tolist() == [3 * i for i in range(22)]
    assert [bin(O.morton_encode(r - 1, r - 1, r - 1)).count("1") for r in (1 << i for i in range(22))] == got[2].tolist()
    assert got[1][0] == -1 and O.bsearch([], 0) == -1 and O.bsearch([5], 5) == 0
    assert got[4].tolist() == [68, 32, 16, 8]
    R.check("helpers", got, walk, lambda w: helper_answers(w.get_hit_n, w.bsearch, w.sort_bits_morton, w.hash_combine, w.struct_sizes))
