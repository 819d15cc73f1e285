"""numpy model of the coarsening (include/mvrt.h, mvrt_svo_coarse_voxels / mvrt_svo_coarsen), written from the semantics alone, two ways that
must agree.

Input: the voxel set as distinct coordinates with one 8-byte attribute each (colour R, G, B, A, emission R, G, B, A).  The coarse cell of (x, y, z) is
(x >> k, y >> k, z >> k); a cell is kept when it holds at least min_count voxels; its attribute is, per channel R, G, B of colour and of emission, the floor of
the exact integer sum over its voxels divided by their number, both alpha bytes 255 (the source's alpha bytes are not read); cells in ascending Morton code."""
import numpy as np

import surface_expected as S

CHANNELS = (0, 1, 2, 4, 5, 6)  # of the 8 attribute bytes: the alpha bytes 3 and 7 are not read


def default_attribs(n):
    """what build_voxels stores for attribs=None: white, no emission"""
    return np.tile(np.array([255, 255, 255, 255, 0, 0, 0, 255], np.uint8), (n, 1))


def _result(xyz, attribs, count):
    return {"xyz": np.asarray(xyz, np.uint32).reshape(-1, 3), "attribs": np.asarray(attribs, np.uint8).reshape(-1, 8), "count": np.asarray(count, np.uint32).reshape(-1)}


def coarse(xyz, attribs, k, min_count=1):
    """grouping by np.unique of the shifted codes, sums by np.add.reduceat in int64"""
    xyz = np.asarray(xyz, np.int64).reshape(-1, 3)
    attribs = default_attribs(len(xyz)) if attribs is None else np.asarray(attribs, np.uint8).reshape(-1, 8)
    codes = S.morton(xyz)
    order = np.argsort(codes, kind="stable")
    assert (np.diff(codes[order].astype(np.int64)) > 0).all(), "the voxel set holds a coordinate twice"
    cell = codes[order] >> np.uint64(3 * k)
    cells, first, count = np.unique(cell, return_index=True, return_counts=True)
    sums = np.add.reduceat(attribs[order].astype(np.int64), first, axis=0)
    out = np.full((len(cells), 8), 255, np.int64)
    for c in CHANNELS:
        out[:, c] = sums[:, c] // count
    keep = count >= min_count
    return _result(S.decode(cells[keep]), out[keep], count[keep])


def coarse_loop(xyz, attribs, k, min_count=1):
    """the same with a plain dictionary: for the small cases"""
    xyz = np.asarray(xyz, np.int64).reshape(-1, 3)
    attribs = default_attribs(len(xyz)) if attribs is None else np.asarray(attribs, np.uint8).reshape(-1, 8)
    assert len({tuple(p) for p in xyz.tolist()}) == len(xyz), "the voxel set holds a coordinate twice"
    cells = {}
    for p, a in zip(xyz.tolist(), attribs.tolist()):
        entry = cells.setdefault((p[0] >> k, p[1] >> k, p[2] >> k), [0] * 7)
        for j, c in enumerate(CHANNELS):
            entry[j] += a[c]
        entry[6] += 1
    kept = [c for c, e in cells.items() if e[6] >= min_count]
    kept.sort(key=lambda c: int(S.morton([c])[0]))
    out = []
    for c in kept:
        e = cells[c]
        m = [e[j] // e[6] for j in range(6)]
        out.append(m[:3] + [255] + m[3:] + [255])
    return _result(kept, out, [cells[c][6] for c in kept])


def same(a, b):
    return all(a[f].shape == b[f].shape and np.array_equal(a[f], b[f]) for f in ("xyz", "attribs", "count"))
