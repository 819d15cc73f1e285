"""Every device allocation of mvrt_svo_walk_voxels and mvrt_svo_rebuild is made to fail in turn (mvrt_test_fail_allocation), like
tests/test_gpu_surface_alloc_failures.py does for the surface calls.  The walk only reads the handle and keeps its scratch in DevBufs: each failure is an
error that names the hook, leaves the uploaded octree bit-identical and tracing as before, the caller's arrays untouched, and mvrt_test_allocation_state
where it was.  A rebuild builds next to the old octree: a failure leaves the handle unchanged, or -- once the new arrays are being adopted, as for every
build -- empty; never half."""
import numpy as np
import pytest

import walk_expected as W
from alloc_sweep import bits, filled, mv, sweep_reader  # noqa: F401 (mv: the fixture)
from edit_model import assert_svo
from fixtures import O  # noqa: F401 (fixtures)
from rays import random_rays
from upload_shapes import oracle_scene, shapes, upload, voxel_set

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def base():
    return voxel_set("random7", 7, 20_000, 2_000, 7)


@pytest.mark.parametrize("emb", [True, False])
def test_each_allocation_of_a_walk_fails_in_turn(mv, O, base, emb):
    nodes = shapes(O, base, emb, 31)["all"][0]
    sc = oracle_scene(O, base, nodes, emb)
    svo = upload(mv, sc, emb)
    paths, vi, xyz = W.walk(nodes, base.res, emb)
    n = len(paths)
    want = {"xyz": xyz, "vIndex": vi, "attribs": sc.attrs[vi]}
    outs = {"xyz": filled(mv, (n, 3), np.uint32), "vIndex": filled(mv, n, np.uint32), "attribs": filled(mv, (n, 8), np.uint8)}
    d = {k: v[0] for k, v in outs.items()}
    ro, rd = random_rays(sc, 6000, 3)
    traced = svo.intersect(ro, rd, want_descents=True)
    # the root entry; offsets and scan storage per level; a frontier per inner level; codes and sums
    total, result = sweep_reader(mv, lambda: svo.walk_voxels_device(n, d["xyz"], d["vIndex"], d["attribs"]), [svo], list(outs.values()), 3 + 2 * 7 + 6 * 3 + 2,
                                 download=lambda h: h.download()[:2])
    print("walk: allocations failed in turn:", total)
    got = svo.intersect(ro, rd, want_descents=True)
    assert all(np.array_equal(got[k], traced[k]) for k in traced)
    assert result == n
    for name in d:
        assert np.array_equal(bits(d[name].to_host()), bits(want[name])), name


@pytest.mark.parametrize("emb,flags", [(True, 0), (False, 1)])
def test_each_allocation_of_a_rebuild_fails_in_turn(mv, O, base, emb, flags):
    nodes = shapes(O, base, emb, 32)["all"][0]
    sc = oracle_scene(O, base, nodes, emb)
    paths, vi, _ = W.walk(nodes, base.res, emb)
    ro, rd = random_rays(sc, 6000, 4)
    svo = upload(mv, sc, emb)
    traced = svo.intersect(ro, rd, want_descents=True)
    info = bytes(svo.info())
    held = mv.allocation_state()[:2]
    unchanged = emptied = 0
    k = 0
    while True:
        k += 1
        assert k < 2000
        mv.set_test_fail_allocation(k)
        try:
            svo.rebuild(flags)
        except mv.MvrtError as e:
            assert "mvrt_test_fail_allocation" in str(e), k
            assert mv.lib().mvrt_test_fail_allocation(0) == 0
            if svo.info().numberOfNodes == 0:  # the new arrays were being adopted: the handle is empty and holds nothing
                emptied += 1
                with pytest.raises(mv.MvrtError, match="no octree"):
                    svo.walk_voxels_device()
                upload(mv, sc, emb, svo)
                assert mv.allocation_state()[:2] == held, k
            else:  # unchanged: the upload, bit for bit, tracing as before, nothing gained
                unchanged += 1
                assert emptied == 0, k  # (failures before the adoption come first)
                assert bytes(svo.info()) == info and mv.allocation_state()[:2] == held, k
                assert np.array_equal(svo.download()[0].view(O.NODE_DTYPE), nodes), k
                got = svo.intersect(ro, rd, want_descents=True)
                assert all(np.array_equal(got[f], traced[f]) for f in traced), k
            continue
        assert mv.lib().mvrt_test_fail_allocation(0) == 0  # (the hook did not fire: fewer than k allocations)
        break
    print("rebuild: allocations failed in turn:", k - 1, "handle unchanged:", unchanged, "emptied:", emptied)
    assert unchanged >= 30 and emptied >= 1
    assert_svo(O, svo, paths, sc.attrs[vi], sc.has_emission, base.res, flags, len(paths))
