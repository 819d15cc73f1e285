"""The CPU oracle (oracle/mvrt_oracle.cpp) against the COMPILED reference, bit for bit: the voxelizer's VTContext, buildOctreeDAGReference /
buildOctreeNaive / embedMask, octreeTraverse_EfficientParametric and the small helpers of voxCommon.hpp, built as they lie into
oracle/_ref/libmvrt_ref_walk.so (oracle/ref_shim_walk.cpp; DESIGN.md section 2 has the flags and the stand-in rule), and -- second half of this
file -- the renderer's sampling code against the host branch of renderCommon.hpp / pmjSampler.hpp in oracle/_ref/libmvrt_ref_render.so.

Every GPU test of this repository is bit-exact against the oracle, and the oracle is a hand-written restatement: a misreading of the reference
shared by the oracle and the kernels would pass everything else.  Where oracle/_ref is absent the oracle must reproduce the SHA-256 of the
reference's answer stored in tests/golden/reference_pin_digests.json (tests/reference_pins.py::check); where the reference tree is present a missing
library or symbol fails.  No tolerance anywhere in the first half; the second states where one applies (math mode 1) and derives it.

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


@pytest.mark.parametrize("scene", R.FAR_SCENES)
def test_traversal_far_origins(walk, scene):
    """60 000 rays at voxels from origins extent * 2^k away, k = 0 .. 23 (R.far_rays): one float32 rounding of a slab time spans up to the whole grid, t reaches
    2^43 extents.  t by its bits, nMajor and vIndex on all of them, a third shadow rays."""
    rs = R.ray_scene(O, scene)
    ro, rd, sh, k = R.far_rays_of(O, scene, R.N_FAR_PIN)
    ext = float((rs.upper - rs.lower).max())
    dist = np.linalg.norm(ro.astype(np.float64) - (rs.lower.astype(np.float64) + rs.upper) / 2, axis=1) / ext
    # the origin is 2^k extents from its target, the target at most sqrt( 3 ) / 2 extents from the centre
    assert len(ro) == R.N_FAR_PIN and set(k.tolist()) == set(range(R.FAR_K)) and (np.abs(dist - 2.0 ** k) <= 0.87 + 2.0 ** k * 1e-6).all()
    got = rs.sc.trace(ro, rd, sh, threads=8)
    hit = got["t"] != R.MAXF
    per_k = np.bincount(k[hit], minlength=R.FAR_K)
    assert (per_k[:6] >= 1000).all() and (per_k > 0).all() and (~hit).sum() >= 1000, per_k  # most near rays hit; hits at every distance; misses
    assert got["t"][hit].max() > 2.0 ** 30 * got["t"][hit].min()
    R.check("trace_far/" + scene, [got["t"], got["nMajor"], got["vIndex"]], walk,
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


# ====================================================================================================================================================
# The renderer's sampling code against the host branch of renderCommon.hpp / pmjSampler.hpp, compiled as they lie into
# oracle/_ref/libmvrt_ref_render.so (oracle/ref_shim_render.cpp).  Math mode 0 (libm): bit for bit.  Math mode 1 (mvrt_detmath.h, what the kernels
# compute): everything free of transcendentals still bit for bit, the rest within bounds derived below.  Answers free of libm also have a stored
# digest (check()); answers that pass through sinf / cosf / atan2f / powf depend on the host's C library -- "host semantics" here is this build's
# glibc, not the MSVC CRT of the reference's own build -- so they have none and skip by name where the library is absent (R.needs_libm).
# ====================================================================================================================================================
@pytest.fixture(scope="module")
def render():
    return R.load_render(O, tree_decides=True)


def same_bits(key, got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (key, k, g.dtype, w.dtype, g.shape, w.shape)
        same = R.bits(g) == R.bits(w)
        assert same.all(), "%s: array %d differs from the compiled reference at %d of %d entries, first at %s" % (key, k, (~same).sum(), same.size, np.argwhere(~same)[0])


def test_render_struct_sizes(render):
    assert O.struct_sizes()["CameraPinhole"] == 60 and O.PMJ_FLOATS == 2 * 4096 * 128
    if render is not None:
        assert render.struct_sizes() == {"CameraPinhole": 60, "PCG32": 16, "PMJ_LENGTH": 4096, "PMJ_N_SEQUENCE": 128}


@pytest.mark.parametrize("thin", [False, True], ids=["shoot", "shootThinLens"])
@pytest.mark.parametrize("cam", ["probe", "skew"])
def test_camera(render, cam, thin):
    """shoot / shootThinLens: corner pixels, offsets and lens samples at 0 and at the float below 1, W != H and odd sizes, and a skewed basis in which no
    product is exact -- so the association of `m_right * mix( ... ) * imageWidth / imageHeight` is settled by the compiled reference.
    No transcendental: the same answer in both math modes."""
    c = R.cameras()[cam]
    px, fl = R.camera_rays()
    assert len(px) > 2500
    got = list(O.RenderOracle(0).camera_shoot(c, px, fl, thin))
    if cam == "skew":
        assert len(np.unique(got[1][:, 0])) > 2000  # the rays differ: the case is no constant
    R.check("render/camera/%s/%d" % (cam, thin), got, render, lambda r: list(r.camera_shoot(c, px, fl, thin)))
    # the per-call entry point the other tests use is the same code
    i = len(px) - 1
    one = O.camera_shoot(c, int(px[i, 0]), int(px[i, 1]), float(fl[i, 0]), float(fl[i, 1]), int(px[i, 2]), int(px[i, 3]), thin, float(fl[i, 2]), float(fl[i, 3]))
    assert np.array_equal(one[0], got[0][i]) and np.array_equal(one[1], got[1][i])


def test_pcg32_uniformf(render):
    seeds = [(0, 2525), (0, 0), (1, 1), (2**64 - 1, 2**64 - 1), (0x0123456789ABCDEF, 2**63)]
    x = np.concatenate([[0, 1, 511, 512, 2**31, 2**32 - 512, 2**32 - 1], np.random.default_rng(75).integers(0, 2**32, 5000)]).astype(np.uint32)

    def answers(r):
        return [np.concatenate([r.pcg32(s, t, 1000) for s, t in seeds]), r.uniformf(x)]
    got = answers(O.RenderOracle(0))
    assert got[1].min() == 0.0 and got[1].max() == np.float32(1 - 2.0 ** -23) == np.float32(O.uniformf(2**32 - 1))  # a float of [1, 2) minus 1
    R.check("render/pcg32_uniformf", got, render, answers)


def test_pmj_table(render):
    """the whole table of PMJSampler::setup( false, ... ), not only its hash"""
    t = O.pmj_table()
    assert R.hashlib.sha256(t.tobytes()).hexdigest().startswith("f6eb7cf3")  # the survey's golden
    R.check("render/pmj_table", [t], render, lambda r: [r.pmj_table()])


def test_sample2d_and_scrambles(render):
    """sample2d over sample indices 0 .. 4095 and beyond, every dimension of kPtGenerate and the shade kernel and dimensions past the 128 sequences,
    streams 0 and 2^32 - 1; nested_uniform_scramble / scramble_f32 on their own.  No transcendental: both math modes."""
    si, di, st = R.sample2d_inputs()
    assert len(si) > 500_000 and di.max() == 2**32 - 1 and set(range(R.PT_DIMENSIONS)) <= set(di.tolist())
    table = O.pmj_table()
    rng = np.random.default_rng(76)
    x = np.concatenate([[0, 1, 2**31, 2**32 - 1, 0x7FFFFF, 0x800000], rng.integers(0, 2**32, 20_000)]).astype(np.uint32)
    seed = np.concatenate([[0, 2**32 - 1, 1, 0, 2**31, 7], rng.integers(0, 2**32, 20_000)]).astype(np.uint32)
    xf = np.concatenate([[0, R.BELOW1, 0.5, 2.0 ** -24, 2.0 ** -23], rng.random(20_001)]).astype(np.float32)

    def answers(r):
        return [r.sample2d(table, si, di, st), r.nested_uniform_scramble(x, seed), r.scramble_f32(xf, seed)]
    got = answers(O.RenderOracle(0))
    assert 0.0 <= got[0].min() and got[0].max() < 1.0
    assert np.array_equal(O.pmj_sample2d(int(si[-7]), int(di[-7]), int(st[-7]), table), got[0][-7])
    R.check("render/sample2d", got, render, answers)


def test_small_helpers(render):
    """rawReflectance and luminance, upper_bound_f (ties: `value <= b` steps past an equal entry; empty and one-element tables), LCGShuffler"""
    rng = np.random.default_rng(77)
    rgba = np.stack(np.meshgrid(np.arange(256), [0, 255, 17], indexing="ij"), -1).reshape(-1, 2)
    rgba = np.stack([rgba[:, 0], rgba[:, 1], 255 - rgba[:, 0], rgba[:, 1]], 1).astype(np.uint8)
    rgb = np.concatenate([rng.random((2000, 3)) * 10, [[0, 0, 0], [1e-45, 1e-45, 1e-45], [3e38, 0, 0]]]).astype(np.float32)
    tables = [np.array([], np.float32), np.array([0.5], np.float32), np.array([0, 0, 0.25, 0.25, 0.25, 1], np.float32), np.sort(rng.random(37)).astype(np.float32)]
    lcg = [(1, 0, 1), (5, 3, 16), (6, 3, 16), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFB), (2654435761, 12345, 97 * 61), (0, 7, 10)]
    idx = np.concatenate([np.arange(100), [2**32 - 1, 2**31]]).astype(np.uint32)

    def answers(r):
        out = [r.reflectance(rgba)[1], r.luminance(rgb)]
        for t in tables:
            b = np.concatenate([t, [0, 1, -1, 0.25, 0.3], rng.random(0)]).astype(np.float32)
            out.append(r.upper_bound(t, b))
        for a, c, n in lcg:
            ok, sh = r.lcg_shuffler(a, c, n, idx)
            out += [np.array([ok], np.uint8), sh]
        return out
    got = answers(O.RenderOracle(0))
    assert got[4].tolist()[:6] == [2, 2, 5, 5, 5, 6]  # an entry equal to b is stepped over
    assert got[6][0] == 1 and got[10][0] == 0 and sorted(got[9][:16].tolist()) == list(range(16))  # gcd( 5, 16 ) == 1: a permutation; gcd( 6, 16 ) != 1
    R.check("render/helpers", got, render, answers)


# ---- libm: compared only against the library -------------------------------------------------------------------------------------------------------
# What test_detmath.py asserts about mvrt_detmath.h against exact values, plus what glibc documents for its float functions (below 1 ulp), gives
# the distance between a math-mode-1 and a libm answer of one call:
#   sin, cos on [-4 pi, 4 pi]    2.5e-7 + 2^-24 (one ulp of a value in [0.5, 1])                              E_T  = 3.1e-7
#   atan2                        1e-6 + 2^-22 (one ulp of a value in [2, 4), pi)                              E_A  = 1.24e-6
#   pow( x, 2.2 ), x in [1/255, 1]   test_detmath.py bounds pow( x, 1 / 2.2 ) on [1e-6, 64] by 2e-6 relative.  pow is exp( y log x ): its relative error is
#                                that of exp plus | y log x | times that of log; | y log x | is at most 6.3 there and 2.2 * log( 255 ) = 12.2 here,
#                                so at most twice the bound, plus one ulp of libm (1.2e-7 relative)               E_P  = 4.2e-6 relative
E_T, E_A, E_P = 3.1e-7, 1.24e-6, 4.2e-6
ULP1 = 2.0 ** -24  # half an ulp of a value below 2 is at most this; a float operation on values below 1 rounds by at most ULP1 / 2


def test_lambert_basis_spherical_degamma(render):
    """math mode 0 against the reference bit for bit: GetOrthonormalBasis and sampleLambertian on +-axes, z = -1 exactly, z = -0 and z a denormal, a in
    {0, 1}, b in {0, the float below 1}; getSpherical on axes, poles and random directions; degammaReflectance on all 256 byte values.
    Math mode 1 within bounds:
      sampleLambertian   x = r cos, y = r sin with r <= 1 differ by E_T each; a component is xaxis_i x + yaxis_i y + Ng_i z with | xaxis_i | + | yaxis_i |
                         <= sqrt 2 for an orthonormal basis: sqrt 2 E_T, and four roundings of values below 1 on either side (8 * 2^-25)   6.8e-7
      getSpherical       u = ( atan2 + PI ) / 2 PI: E_A, the rounding of atan2's sum with PI, a value below 8, on either side (at most 2^-22 each,
                         4 * 2^-23 together), all over 2 PI, and the division's roundings (2 * 2^-25): 3.3e-7.  v = atan2 / PI: E_A / PI + 2 * 2^-25: 4.6e-7
      degammaReflectance E_P relative"""
    R.needs_libm(render, "sampleLambertian / getSpherical / degammaReflectance")
    ab, n = R.lambert_inputs()
    assert len(ab) > 20_000
    dirs = np.concatenate([R.SPECIAL_NORMALS, np.array([[0, 0, 0], [1e-45, 0, 1e-45], [-1, 0, 1e-45], [-1, 0, -1e-45], [3e38, 1, 3e38]], np.float32), R.unit_normals(20_000, 78)])
    rgba = np.stack([np.arange(256)] * 4, 1).astype(np.uint8)

    def answers(r):
        return list(r.orthonormal_basis(n)) + [r.sample_lambertian(ab, n), r.get_spherical(dirs), r.reflectance(rgba)[0]]
    want = answers(render)
    got0 = answers(O.RenderOracle(0))
    same_bits("render/lambert", got0, want)
    assert np.array_equal(O.sample_lambertian(float(ab[-1, 0]), float(ab[-1, 1]), n[-1], 0), got0[2][-1])
    got1 = answers(O.RenderOracle(1))
    same_bits("render/basis (math mode 1)", got1[:2], want[:2])  # no transcendental
    fin = np.isfinite(want[3]).all(1)
    err = {"lambert": np.abs(got1[2].astype(np.float64) - want[2]).max(), "spherical_u": np.abs(got1[3][fin, 0].astype(np.float64) - want[3][fin, 0]).max(),
           "spherical_v": np.abs(got1[3][fin, 1].astype(np.float64) - want[3][fin, 1]).max(),
           "degamma": (np.abs(got1[4][1:].astype(np.float64) - want[4][1:]) / want[4][1:]).max()}
    print("math mode 1 against the reference, measured maxima:", err)
    assert err["lambert"] <= np.sqrt(2) * E_T + 8 * 2.0 ** -25
    assert err["spherical_u"] <= (E_A + 4 * 2.0 ** -23) / (2 * np.pi) + 2 * 2.0 ** -25
    assert err["spherical_v"] <= E_A / np.pi + 2 * 2.0 ** -25
    assert err["degamma"] <= E_P and (got1[4][0] == 0).all() and (want[4][0] == 0).all()
    assert np.array_equal(np.isfinite(got1[3]), np.isfinite(want[3]))


# Tables without a total (all zeros; 1 .. 6 = +x, -x, +y, -y, +z, -z), in both math modes.  The cosine weight of a table is taken at the texel's centre: a
# one-row map has all its centres on the horizon (nothing for +-y), a one-column map has its centres at phi = 2 PI, direction +x (nothing for -x, and for
# +-z only the sign of sin( fl( 2 PI ) ) = +1.7e-7 decides: +z keeps a total, -z does not); black_ground has no light below the horizon.
NO_TOTAL = {"noise1x1": {2, 3, 4, 6}, "noise2x1": {3, 4}, "noise1x2": {2, 6}, "black_ground": {4}}


def hdri_answers(render, name, math_mode):
    """(N, u, which table per call, the oracle's HDRI, its seven tables, got = (direction, L, srPDF) per axisAligned, want the same from the reference on
    the oracle's tables, or None without the library).  Calls whose table has no total go to the oracle only."""
    rgba, w, h = R.hdri_map(name)
    hd = O.HDRI(rgba, w, h, math_mode=math_mode)
    hd.set_scale(1.75)
    tabs = [hd.sat(k) for k in range(7)]
    N, u = R.hdri_inputs(tabs, w, h)
    which = R.table_of_normal(N)
    got, want = {}, {}
    for aa in (True, False):
        got[aa] = hd.importance_sample_batch(N, u, aa)
        ok = np.array([tabs[t][-1] != 0 for t in (which if aa else np.zeros_like(which))])
        if render is not None:
            want[aa] = (ok, render.hdri_importance_sample(rgba, w, h, tabs, 1.75, N[ok], u[ok], aa))
    return rgba, w, h, hd, tabs, N, u, which, got, (want if render is not None else None)


@pytest.mark.parametrize("name", R.HDRI_MAPS)
def test_importance_sample_libm(render, name):
    """HDRI::importanceSample in math mode 0, bit for bit: direction, L and srPDF on every map, with and without axisAligned, normals on both sides of
    the 0.8 threshold of every axis (0.8 itself included), u0 / u1 at 0, below 1 and on table entries, u2 / u3 at 0 and below 1.  The tables are the
    oracle's own, handed to the reference (it builds its tables in voxKernel.cu, which no host compiler builds)."""
    R.needs_libm(render, "importanceSample's direction and srPDF")
    rgba, w, h, hd, tabs, N, u, which, got, want = hdri_answers(render, name, 0)
    assert len(N) > 1500 and set(which.tolist()) == set(range(7))
    for aa in (True, False):
        ok, ref = want[aa]
        assert ok.sum() > (0.3 if name in NO_TOTAL and aa else 0.8) * len(ok) and (aa or ok.all())
        same_bits("render/importanceSample/%s/%d" % (name, aa), [a[ok] for a in got[aa]], list(ref))
    assert np.array_equal(hd.importance_sample(N[5], u[5], True)[0], got[True][0][5])


def table_points(w, h, seed):
    rng = np.random.default_rng(seed)
    xs = np.unique(np.concatenate([[0, 1, w - 1, w], rng.integers(0, w + 1, 40)]))
    ys = np.unique(np.concatenate([[0, 1, h - 1, h], rng.integers(0, h + 1, 40)]))
    return np.stack(np.meshgrid(xs, ys, indexing="ij"), -1).reshape(-1, 2).astype(np.uint32)


@pytest.mark.parametrize("math_mode", [0, 1])
@pytest.mark.parametrize("name", R.HDRI_MAPS)
def test_importance_sample_selection(render, name, math_mode):
    """what importanceSample computes without a transcendental, in BOTH math modes and bit for bit: the selected texel (read back as L -- the noise maps have
    no two equal pixels), getPrefixSumExclusiveH / V and getCount of all seven tables.  Given the tables, nothing here depends on libm; the tables are
    the oracle's, and those of math mode 0 are built with the host's libm.  So math mode 1 has stored digests, and math mode 0 is compared with the library
    only and skips by name without it.
    Math mode 1's direction and srPDF are compared within bounds:
      sY = mix( cos t0, cos t1, u2 )  E_T (a convex combination of two errors of at most E_T) and three roundings on either side: D_Y = E_T + 6 * 2^-25
      sinTheta = sqrt( max( 1 - sY^2, 0 ) )   1 - sY^2 moves by at most D_1 = 2 D_Y + 2 * 2^-24, and | sqrt a - sqrt b | <= min( sqrt | a - b |, | a - b | / sqrt a ):
                         D_S = min( sqrt D_1, D_1 / sinTheta of the reference ) + 2^-24, per sample (near the poles the square root is ill-conditioned)
      direction.x, .z = cos / sin( phi ) * sinTheta, phi in [ PI, 3 PI ]:  D_S + E_T + 2 * 2^-25
      srPDF = pSelection / ( dH dPhi ), dH = 2 sin( dTheta / 2 ) sin( dTheta / 2 + theta ), both sines at least sin( dTheta / 2 ): relative
                         2 E_T / sin( dTheta / 2 ) + 6 * 2^-24 (three roundings on either side)"""
    rgba, w, h, hd, tabs, N, u, which, got, want = hdri_answers(render, name, math_mode)
    pts = table_points(w, h, 79)
    key = "render/selection/%s/%d" % (name, math_mode)
    queries = [a for k in range(7) for a in hd.table_queries(k, pts)]
    L = [got[aa][1] for aa in (True, False)]
    # a table without a total: the reference's X = upper_bound - 1 is w - 1 (every prefix is 0 <= u0), vol is 0, 0 / 0 <= u1 is false in every step, so its
    # Y = 0 - 1 wraps to 0xFFFFFFFF and getCount / m_pixels index out of range: undefined, never called.  Those calls must take the oracle's documented
    # "selects nothing" path: direction = N, L = 0, srPDF = 1.  Which: the tables of NO_TOTAL, taken by the normals past 0.8 on that axis, with axisAligned
    # only (the uniform table of every map here has a total).  Every other table ends in 0xFFFFFFFF, and then the reference is defined for every u in
    # [0, 1): prefix( 0 ) = 0 <= u keeps upper_bound at 1 or more (X, Y >= 0), and the last prefix, 0xFFFFFFFF / 0xFFFFFFFF = vol / vol = 1 > u, keeps it in range.
    dead = np.array([tabs[t][-1] == 0 for t in which])
    assert set(which[dead].tolist()) == NO_TOTAL.get(name, set())
    d, l, p = got[True]
    assert np.array_equal(d[dead], N[dead]) and (l[dead] == 0).all() and (p[dead] == 1).all()
    assert all(t[-1] == (0 if k in NO_TOTAL.get(name, set()) else 0xFFFFFFFF) for k, t in enumerate(tabs))
    if name.startswith("noise"):
        assert len(np.unique(rgba[:, :3], axis=0)) == w * h  # L names the texel
    if math_mode == 0 and render is None:
        pytest.skip("the math-mode-0 tables depend on the host's libm: compared only where oracle/_ref/libmvrt_ref_render.so is present")

    def reference(r):
        out = [a for k in range(7) for a in r.hdri_table_queries(tabs[k], w, h, pts)]
        for aa in (True, False):
            ok = ~dead if aa else np.ones(len(N), bool)
            ref_l = np.zeros_like(got[aa][1])
            ref_l[ok] = r.hdri_importance_sample(rgba, w, h, tabs, 1.75, N[ok], u[ok], aa)[1]
            out.append(ref_l)
        return out
    if math_mode == 0:
        same_bits(key, queries + L, reference(render))
        return
    R.check(key, queries + L, render, reference)
    if render is None:
        return
    d_y = E_T + 6 * 2.0 ** -25
    d_1 = 2 * d_y + 2 * 2.0 ** -24
    worst = {"sY": 0.0, "xz over its bound": 0.0, "srPDF relative": 0.0}
    for aa in (True, False):
        ok, (rd, rl, rp) = want[aa]
        gd, gp = got[aa][0][ok].astype(np.float64), got[aa][2][ok].astype(np.float64)
        sin_ref = np.hypot(rd[:, 0].astype(np.float64), rd[:, 2].astype(np.float64))
        d_s = np.minimum(np.sqrt(d_1), d_1 / np.maximum(sin_ref, 1e-30)) + 2.0 ** -24
        bound_xz = d_s + E_T + 2 * 2.0 ** -25
        e_y = np.abs(gd[:, 1] - rd[:, 1])
        e_xz = np.maximum(np.abs(gd[:, 0] - rd[:, 0]), np.abs(gd[:, 2] - rd[:, 2]))
        pos = rp > 0
        e_p = np.abs(gp[pos] - rp[pos]) / rp[pos]
        worst["sY"] = max(worst["sY"], e_y.max())
        worst["xz over its bound"] = max(worst["xz over its bound"], (e_xz / bound_xz).max())
        worst["srPDF relative"] = max(worst["srPDF relative"], e_p.max() if pos.any() else 0.0)
        bound_p = 2 * E_T / np.sin(np.pi / h / 2) + 6 * 2.0 ** -24
        print("%s axisAligned %d, math mode 1 against the reference: sY %.3g (bound %.3g), x/z at most %.3g of the per-sample bound, srPDF relative %.3g (bound %.3g)"
              % (name, aa, e_y.max(), d_y, (e_xz / bound_xz).max(), e_p.max() if pos.any() else 0.0, bound_p))
        assert (e_y <= d_y).all() and (e_xz <= bound_xz).all() and (e_p <= bound_p).all()
        assert np.array_equal(gp[~pos], rp[~pos].astype(np.float64))
