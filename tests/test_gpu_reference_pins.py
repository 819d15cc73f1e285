"""The HIP kernels against the COMPILED reference directly (oracle/_ref/libmvrt_ref_walk.so; never the reference tree): the voxelizer and the builder
on the triangles where voxelizers go wrong -- vertices on lattice points, triangles in lattice planes, equal vertices, slivers, clipped and sub-voxel
triangles -- and the traversal on the ray set of tests/test_reference_pins_cpu.py.  The other GPU tests compare with the oracle, which is a restatement
of the reference written together with the kernels; these do not go through it.  Where oracle/_ref is absent the kernels must reproduce the stored
SHA-256 of the reference's answer (tests/reference_pins.py::check).  All comparisons are exact.

Colours and emission are compared with the oracle, as everywhere: the reference's barycentric code (closestBarycentricCoordinateOnTriangle) sits in
voxKernel.cu, which no host compiler here builds."""
import numpy as np
import pytest

import reference_pins as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def mv():
    import massivevoxelraytracing_amd as m
    m.lib()
    assert m.device_count() >= 1
    return m


@pytest.fixture(scope="module")
def walk(O):
    return R.load_walk(O, tree_decides=False)


def build_and_compare(mv, O, walk, key, tris, origin, dps, res, flags):
    cols, emis = R.vertex_attributes(len(tris), 41)
    svo = mv.IntersectorOctreeGPU()
    svo.build(tris.reshape(-1, 3), cols.reshape(-1, 3), emis.reshape(-1, 3), None, origin, dps, res, flags=flags)
    info = svo.info()
    nodes, attrs, morton = svo.download(want_morton=True)
    nodes = nodes.view(O.NODE_DTYPE)
    assert info.numberOfVoxels == len(morton) and info.numberOfNodes == len(nodes)
    R.check(key, [np.array([info.totalDumpedVoxels], np.uint64), morton] + R.node_fields(nodes), walk,
            lambda w: R.reference_build(w, tris, origin, dps, res, flags))
    # attributes: the oracle's, merged like the reference's `unique` kernel merges them
    m, a = O.voxelize(tris, origin, dps, res, cols, emis, six_separating=not (flags & R.CONSERVATIVE))
    m, a, he = O.merge_voxels(m, a)
    assert np.array_equal(m, morton) and np.array_equal(a, attrs) and info.hasEmission == he


CLASS_CASES = R.class_build_cases()


@pytest.mark.parametrize("case", CLASS_CASES, ids=[c[0] for c in CLASS_CASES])
def test_triangle_class_builds(mv, O, walk, case):
    """dumped count, the sorted unique voxel list and the embedded DAG nodes of each class (plus one ordinary triangle), 32^3 and 4^3, six-separating
    and conservative"""
    build_and_compare(mv, O, walk, *case)


@pytest.mark.parametrize("flags", [0, R.CONSERVATIVE])
@pytest.mark.parametrize("res", [32, 4])
def test_equal_vertices_alone_touch_no_voxel(mv, res, flags):
    """the reference finds no voxel for a triangle with two equal vertices (tests/test_reference_pins_cpu.py asserts the counts are 0); a mesh of nothing
    else is refused by name"""
    origin, dps = R.class_grid(res)
    tris = R.triangle_classes(res)["two_equal"]
    svo = mv.IntersectorOctreeGPU()
    with pytest.raises(mv.MvrtError, match="touch no voxel"):
        svo.build(tris.reshape(-1, 3), None, None, None, origin, dps, res, flags=flags)


MIXED_CASES = R.mixed_build_cases()


@pytest.mark.parametrize("case", MIXED_CASES, ids=[c[0] for c in MIXED_CASES])
def test_all_classes_between_bunny_triangles(mv, O, walk, case):
    """every class dealt between 3000 bunny triangles at 256^3, footprints on both sides of the whole-wave threshold: the lane-own and the whole-wave path
    of kVoxelize run in the same waves"""
    tris, origin, dps, res = case[1:5]
    v = tris.reshape(-1, 3, 3)
    lo = np.clip(np.floor((v.min(1) - origin) / dps), 0, res - 1)
    hi = np.clip(np.floor((v.max(1) - origin) / dps), 0, res - 1)
    ext = np.sort(hi - lo + 1, axis=1)
    assert (ext[:, 0] * ext[:, 1] > 2048).sum() > 20 and (ext[:, 1] * ext[:, 2] <= 2048).sum() > 3000  # whatever the major axis: some big, most small
    build_and_compare(mv, O, walk, *case)


@pytest.mark.parametrize("scene", ["bunny64", "deep21"])
def test_trace_batch(mv, O, walk, scene):
    """one mvrt_trace_batch of the CPU pin's whole ray set -- ties, origins on voxel corners / edges / faces, secondary-style origins, direction
    components of +-0, denormals, +-inf and NaN, a third shadow rays -- against the reference's traversal: t by its bits, nMajor and vIndex on all rays"""
    rs = R.ray_scene(O, scene)
    ro, rd, sh = R.rays_of(O, scene)
    svo = mv.IntersectorOctreeGPU()
    svo.upload(rs.nodes, rs.sc.attrs, rs.sc.origin, rs.sc.dps, rs.sc.grid_res, rs.sc.has_emission)
    info = svo.info()
    assert np.array_equal(np.array(info.lower[:], np.float32), rs.lower) and np.array_equal(np.array(info.upper[:], np.float32), rs.upper)
    got = svo.intersect(ro, rd, sh)
    R.check("trace/" + scene, [got["t"], got["nMajor"], got["vIndex"]], walk,
            lambda w: [x for x in w.trace(rs.nodes, rs.lower, rs.upper, ro, rd, sh).values()])
