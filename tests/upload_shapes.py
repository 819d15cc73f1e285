"""Octrees of shapes this library's builder never makes, for mvrt_svo_upload (tests/test_upload_shapes_cpu.py, tests/test_gpu_upload_shapes.py).

Everything works on oracle.NODE_DTYPE arrays (the reference's 68-byte nodes, root last) and is seeded:
- legal shapes: `permute` (any numbering, root last), `add_unreachable` (copies and fresh nodes nobody references), `unshare` (DAG -> tree),
  `add_empty_inner` (reachable nodes of mask 0) and the nVoxelsPSum variants `psum_zero`, `psum_random`, `psum_one_off`;
- `check_model`: a plain-Python statement of the upload contract (include/mvrt.h, rules 1-5), independent of the library's checker;
- `voxel_paths`: the root->voxel path (= Morton code) of every voxel, the hints of the GPU tests;
- `MUTATIONS`: single changes that break one rule each.

An octree here is the tuple (nodes, numberOfVoxels, gridRes, embedded).

The last section is what the tests of uploaded octrees build on: the voxel sets (`Base`, `voxel_set`, the `bases` fixture), every legal shape of one of them
(`shapes`), its oracle scene and its upload."""
import numpy as np
import pytest

import deep_scenes as D
from common import bunny_tris, position_colors
from massivevoxelraytracing_amd import IntersectorOctreeGPU

LEAF = 0xFFFFFFFF
IDX = 0xFFFFFF
MAX_RES = 1 << 21


def levels_of(res):
    return int(res).bit_length() - 1


def _index(word, embedded):
    return word & IDX if embedded else word


def _word(idx, masks, embedded):
    """child word of a pointer to node idx (masks: indexable own masks)"""
    return (idx | (int(masks[idx]) << 24)) if embedded else idx


def set_masks_zero_padding(nodes):
    """the three bytes after the mask are not kept by the library (mvrt_svo_download writes 0): the generators write 0"""
    nodes["_pad"][:] = 0
    return nodes


# ---- legal shapes ------------------------------------------------------------------------------------------------------------------------------
def remap(nodes, new_of_old, embedded):
    """renumber: node i moves to new_of_old[i]; child words follow, embedded mask bytes are kept"""
    new_of_old = np.asarray(new_of_old, np.int64)
    out = np.zeros(len(nodes), nodes.dtype)
    out[new_of_old] = nodes
    ch = out["children"].astype(np.int64)
    is_node = ch != LEAF
    idx = np.where(is_node, ch & IDX if embedded else ch, 0)
    hi = ch & 0xFF000000 if embedded else 0
    out["children"] = np.where(is_node, new_of_old[idx] | hi, LEAF).astype(np.uint32)
    return out


def permute(nodes, embedded, rng):
    """a random numbering with the root last"""
    n = len(nodes)
    new_of_old = np.empty(n, np.int64)
    new_of_old[: n - 1] = rng.permutation(n - 1)
    new_of_old[n - 1] = n - 1
    return remap(nodes, new_of_old, embedded)


def insert_before_root(nodes, extra, embedded):
    """nodes + extra with the root moved to the end: words pointing to the old root index are renumbered (extra's words already use the final
    numbering, the root at len(nodes) + len(extra) - 1)"""
    n, k = len(nodes), len(extra)
    new_of_old = np.arange(n, dtype=np.int64)
    new_of_old[n - 1] = n - 1 + k
    body = remap(np.concatenate([nodes, np.zeros(k, nodes.dtype)]), np.concatenate([new_of_old, np.arange(n - 1, n - 1 + k)]), embedded)
    body[n - 1: n - 1 + k] = extra
    return body


def add_unreachable(nodes, embedded, rng, n_copies=3, n_fresh=3):
    """copies of random nodes (their words stay valid) and fresh nodes of random masks whose children are voxels or any node in range, with
    random nVoxelsPSum; nothing points to any of them"""
    n = len(nodes)
    total = n + n_copies + n_fresh
    masks = np.concatenate([nodes["mask"][: n - 1], np.zeros(n_copies + n_fresh, np.uint8), nodes["mask"][n - 1:]])
    copies = nodes[rng.integers(0, n, n_copies)].copy()
    masks[n - 1: n - 1 + n_copies] = copies["mask"]
    fresh = np.zeros(n_fresh, nodes.dtype)
    fresh["mask"] = rng.integers(0, 256, n_fresh)
    masks[n - 1 + n_copies: n - 1 + n_copies + n_fresh] = fresh["mask"]
    # copies point where the originals point: renumber a pointer to the root
    for e in copies:
        for c in range(8):
            w = int(e["children"][c])
            if w != LEAF and _index(w, embedded) == n - 1:
                e["children"][c] = _word(total - 1, masks, embedded)
    for e in fresh:
        e["psum"] = rng.integers(0, 2**32, 8, dtype=np.uint64).astype(np.uint32)
        for c in range(8):
            if (int(e["mask"]) >> c) & 1 and rng.random() < 0.6:
                e["children"][c] = _word(int(rng.integers(0, total)), masks, embedded)
            else:
                e["children"][c] = LEAF
    return insert_before_root(nodes, np.concatenate([copies, fresh]), embedded)


def unshare(nodes, embedded):
    """DAG -> tree: every path gets its own nodes (children numbered before their parent, root last)"""
    masks, ch, ps = nodes["mask"].tolist(), nodes["children"].tolist(), nodes["psum"].tolist()
    out_mask, out_ch, out_ps = [], [], []

    def copy(i):
        kids = []
        for w in ch[i]:
            kids.append(LEAF if w == LEAF else copy(_index(w, embedded)))
        words = [LEAF if k == LEAF else (k | (out_mask[k] << 24) if embedded else k) for k in kids]
        out_mask.append(masks[i])
        out_ch.append(words)
        out_ps.append(ps[i])
        return len(out_mask) - 1

    copy(len(nodes) - 1)
    out = np.zeros(len(out_mask), nodes.dtype)
    out["mask"], out["children"], out["psum"] = out_mask, out_ch, out_ps
    return out


def depths(nodes, embedded):
    """depth of every reachable node (-1: unreachable), for octrees that keep rule 3"""
    d = np.full(len(nodes), -1, np.int64)
    cur = np.array([len(nodes) - 1])
    level = 0
    while len(cur):
        d[cur] = level
        ch = nodes["children"][cur].astype(np.int64).reshape(-1)
        ch = ch[ch != LEAF]
        cur = np.unique(ch & IDX if embedded else ch)
        level += 1
    return d


def add_empty_inner(nodes, res, embedded, rng, count=4):
    """reachable nodes of mask 0: a clear slot of a node above the parents of voxels points to a fresh empty node; the embedded bytes of every
    pointer to a changed node follow its new mask"""
    d = depths(nodes, embedded)
    cand = [i for i in np.nonzero((d >= 0) & (d <= levels_of(res) - 2))[0].tolist() if nodes["mask"][i] != 0xFF]
    if not cand:
        return nodes.copy()
    picks = rng.choice(cand, min(count, len(cand)), replace=False).tolist()
    n = len(nodes)
    out = insert_before_root(nodes, np.zeros(len(picks), nodes.dtype), embedded)
    out["children"][n - 1: n - 1 + len(picks)] = LEAF
    new_of_old = lambda i: i if i < n - 1 else i + len(picks)
    for j, p in enumerate(picks):
        p = new_of_old(p)
        free = [c for c in range(8) if not (int(out["mask"][p]) >> c) & 1]
        c = int(rng.choice(free))
        out["mask"][p] |= np.uint8(1 << c)
        out["children"][p, c] = _word(n - 1 + j, out["mask"], embedded)
    if embedded:  # pointers carry the (changed) masks
        ch = out["children"].astype(np.int64)
        is_node = ch != LEAF
        idx = np.where(is_node, ch & IDX, 0)
        out["children"] = np.where(is_node, idx | (out["mask"][idx].astype(np.int64) << 24), LEAF).astype(np.uint32)
    return out


def psum_zero(nodes):
    out = nodes.copy()
    out["psum"] = 0
    return out


def psum_random(nodes, n_voxels, res, rng):
    """random nVoxelsPSum whose sum along any path of log2(res) levels stays below n_voxels (rule 4)"""
    out = nodes.copy()
    cap = max(0, (int(n_voxels) - 1) // levels_of(res))
    out["psum"] = rng.integers(0, cap + 1, out["psum"].shape)
    return out


def psum_one_off(nodes, embedded, rng=None):
    """canonical except one parent of voxels: the value of its last voxel slot (slot 7 where there is one) is lowered by one -- the library's
    popcount shortcut for the last level must turn off while almost every path keeps the canonical sums"""
    out = nodes.copy()
    ch = out["children"]
    voxel_slots = (ch == LEAF) & ((out["mask"][:, None] >> np.arange(8)) & 1).astype(bool)
    d = depths(out, embedded)
    ok = (voxel_slots.sum(1) >= 2) & (d >= 0)
    with7 = np.nonzero(ok & voxel_slots[:, 7])[0]
    cand = with7 if len(with7) else np.nonzero(ok)[0]
    assert len(cand), "no parent of two voxels"
    p = int(cand[0] if rng is None else rng.choice(cand))
    c = int(np.nonzero(voxel_slots[p])[0][-1])
    assert out["psum"][p, c] > 0
    out["psum"][p, c] -= 1
    return out, p, c


# ---- the contract, in plain Python -------------------------------------------------------------------------------------------------------------
def check_model(nodes, n_voxels, res, embedded):
    """(accepted, rule, node): rule and first offending node in the library's order (1, 5, then 2 over the nodes in index order, then one walk
    from the root level by level, nodes in the order they are first reached, for 3 and 4); rule / node None where they do not apply"""
    res = int(res)
    if res < 2 or res > MAX_RES or res & (res - 1):
        return False, 1, None
    n = len(nodes)
    if embedded and n >= IDX:
        return False, 5, None
    masks = [int(m) for m in nodes["mask"].tolist()]
    kids = nodes["children"].tolist()
    sums = nodes["psum"].tolist()
    for i in range(n):
        for c, w in enumerate(kids[i]):
            if w == LEAF:
                continue
            if not masks[i] >> c & 1:
                return False, 2, i
            k = w & IDX if embedded else w
            if k >= n or (embedded and w >> 24 != masks[k]):
                return False, 2, i
    L = levels_of(res)
    depth = {n - 1: 0}
    best = {n - 1: 0}
    level = [n - 1]
    over = None
    for dd in range(L + 1):
        nxt = []
        for i in level:
            for c in range(8):
                if not masks[i] >> c & 1:
                    continue
                w = kids[i][c]
                s = best[i] + sums[i][c]
                if w == LEAF:
                    if dd != L - 1:
                        return False, 3, i
                    if s >= n_voxels and over is None:
                        over = i
                    continue
                if dd >= L - 1:
                    return False, 3, i
                k = w & IDX if embedded else w
                if k in depth:
                    if depth[k] != dd + 1:
                        return False, 3, i
                    best[k] = max(best[k], s)
                else:
                    depth[k] = dd + 1
                    best[k] = s
                    nxt.append(k)
        level = nxt
    if over is not None:
        return False, 4, over
    return True, None, None


def max_path_sum(nodes, embedded):
    """(largest nVoxelsPSum sum along a root->voxel path, its parent node, slot) of an octree that keeps rules 2 and 3; (-1, None, None) if empty"""
    masks, kids, sums = nodes["mask"].tolist(), nodes["children"].tolist(), nodes["psum"].tolist()
    best = {len(nodes) - 1: 0}
    level = [len(nodes) - 1]
    top = (-1, None, None)
    while level:
        nxt = []
        for i in level:
            for c in range(8):
                if not masks[i] >> c & 1:
                    continue
                w, s = kids[i][c], best[i] + sums[i][c]
                if w == LEAF:
                    if s > top[0]:
                        top = (s, i, c)
                    continue
                k = _index(w, embedded)
                if k not in best:
                    nxt.append(k)
                    best[k] = s
                best[k] = max(best[k], s)
        level = nxt
    return top


def voxel_paths(nodes, res, embedded):
    """the root->voxel path (3 bits per level, the root's slot highest; = Morton code of the cell) of every voxel of an octree that keeps rules
    2 and 3, sorted, uint64"""
    L = levels_of(res)
    cur_n = np.array([len(nodes) - 1], np.int64)
    cur_p = np.zeros(1, np.uint64)
    for lvl in range(L):
        nn, pp = [], []
        m = nodes["mask"][cur_n].astype(np.int64)
        ch = nodes["children"][cur_n].astype(np.int64)
        for c in range(8):
            sel = (m >> c) & 1 == 1
            nn.append(ch[sel, c])
            pp.append((cur_p[sel] << np.uint64(3)) | np.uint64(c))
        cur_n, cur_p = np.concatenate(nn), np.concatenate(pp)
        if lvl + 1 < L:
            cur_n = cur_n & IDX if embedded else cur_n
    return np.sort(cur_p)


# ---- mutations that break one rule -------------------------------------------------------------------------------------------------------------
def _node_slots(nodes, embedded, want, depth_ok=None):
    """reachable (node, slot) pairs whose child is a node (want='node'), a voxel ('voxel') or absent ('absent')"""
    d = depths(nodes, embedded)
    out = []
    for i in np.nonzero(d >= 0)[0].tolist():
        if depth_ok is not None and not depth_ok(int(d[i])):
            continue
        m = int(nodes["mask"][i])
        for c in range(8):
            w = int(nodes["children"][i, c])
            kind = "absent" if not m >> c & 1 else ("voxel" if w == LEAF else "node")
            if kind == want:
                out.append((i, c))
    return out


def _pick(rng, xs):
    return xs[int(rng.integers(0, len(xs)))] if xs else None


def mut_child_out_of_range(t, rng):
    nodes, nv, res, emb = t
    s = _pick(rng, _node_slots(nodes, emb, "node"))
    if s is None:
        return None
    out = nodes.copy()
    k = int(rng.integers(len(nodes), min(IDX, len(nodes) + 1000)))
    out["children"][s] = (k | (int(out["children"][s]) & 0xFF000000)) if emb else k
    return out, nv, res, emb, 2


def mut_child_out_of_range_unreachable(t, rng):
    nodes, nv, res, emb = t
    out = add_unreachable(nodes, emb, rng, 1, 0)
    i = len(out) - 2
    out["mask"][i] |= 1
    out["children"][i, 0] = len(out) + int(rng.integers(0, 50))
    return out, nv, res, emb, 2


def mut_garbage_in_absent_slot(t, rng):
    nodes, nv, res, emb = t
    s = _pick(rng, _node_slots(nodes, emb, "absent"))
    if s is None:
        return None
    out = nodes.copy()
    out["children"][s] = int(rng.choice([0, 1, len(nodes) - 1, int(rng.integers(0, 2**32 - 1))]))
    return out, nv, res, emb, 2


def mut_wrong_embedded_byte(t, rng):
    nodes, nv, res, emb = t
    s = _pick(rng, _node_slots(nodes, emb, "node"))
    if not emb or s is None:
        return None
    out = nodes.copy()
    w = int(out["children"][s])
    out["children"][s] = (w & IDX) | ((((w >> 24) + int(rng.integers(1, 256))) & 0xFF) << 24)
    return out, nv, res, emb, 2


def mut_plain_indices_as_embedded(t, rng):
    nodes, nv, res, emb = t
    if not emb or not _node_slots(nodes, emb, "node"):
        return None
    out = nodes.copy()
    ch = out["children"]
    out["children"] = np.where(ch == LEAF, ch, ch & np.uint32(IDX))
    return out, nv, res, emb, 2


def mut_self_loop(t, rng):
    nodes, nv, res, emb = t
    s = _pick(rng, _node_slots(nodes, emb, "node"))
    if s is None:
        return None
    out = nodes.copy()
    out["children"][s] = _word(s[0], out["mask"], emb)
    return out, nv, res, emb, 3


def mut_loop_to_ancestor(t, rng):
    nodes, nv, res, emb = t
    s = _pick(rng, _node_slots(nodes, emb, "node", lambda d: d >= 1) + _node_slots(nodes, emb, "voxel", lambda d: d >= 1))
    if s is None:
        return None
    out = nodes.copy()
    out["children"][s] = _word(len(nodes) - 1, out["mask"], emb)  # the root is every node's ancestor
    return out, nv, res, emb, 3


def mut_coarse_voxel(t, rng):
    nodes, nv, res, emb = t
    s = _pick(rng, _node_slots(nodes, emb, "node"))
    if s is None:
        return None
    out = nodes.copy()
    out["children"][s] = LEAF  # a voxel in place of a subtree: a voxel of 2^k cells per side
    return out, nv, res, emb, 3


def mut_grid_halved(t, rng):
    nodes, nv, res, emb = t
    return nodes, nv, res // 2, emb, 3 if res >= 4 else 1


def mut_grid_doubled(t, rng):
    nodes, nv, res, emb = t
    return nodes, nv, res * 2, emb, 3 if res < MAX_RES else 1


def mut_grid_2_22(t, rng):
    nodes, nv, res, emb = t
    return nodes, nv, 1 << 22, emb, 1


# gridRes values a corrupt file header may hold: every int32 must be answered (rule 1), none may hang the check
GARBAGE_GRID_RES = (0, 1, 3, -4, -(1 << 31), (1 << 31) - 1, 1 << 30, (1 << 30) + 1, (1 << 29) * 3, (1 << 21) + 1, (1 << 21) - 1, 1 << 22)


def mut_grid_garbage(t, rng):
    nodes, nv, res, emb = t
    v = GARBAGE_GRID_RES[int(rng.integers(0, len(GARBAGE_GRID_RES)))] if rng.random() < 0.5 else int(rng.integers(-(1 << 31), 1 << 31))
    if v >= 2 and v <= MAX_RES and not v & (v - 1):
        v = -v
    return nodes, nv, v, emb, 1


def mut_node_at_two_depths(t, rng):
    nodes, nv, res, emb = t
    d = depths(nodes, emb)
    pairs = [(i, c) for (i, c) in _node_slots(nodes, emb, "node") if (d == d[i] + 2).any()]
    s = _pick(rng, pairs)
    if s is None:
        return None
    far = np.nonzero(d == d[s[0]] + 2)[0]
    out = nodes.copy()
    out["children"][s] = _word(int(far[int(rng.integers(0, len(far)))]), out["mask"], emb)
    return out, nv, res, emb, 3


def mut_psum_reaches_count(t, rng):
    nodes, nv, res, emb = t
    top, p, c = max_path_sum(nodes, emb)
    if p is None or top >= nv or int(nodes["psum"][p, c]) + nv - top >= 2**32:
        return None
    out = nodes.copy()
    out["psum"][p, c] += nv - top
    return out, nv, res, emb, 4


def mut_voxels_without_count(t, rng):
    nodes, nv, res, emb = t
    if max_path_sum(nodes, emb)[1] is None:
        return None
    return nodes, 0, res, emb, 4


MUTATIONS = {
    "child_out_of_range": mut_child_out_of_range,
    "child_out_of_range_unreachable": mut_child_out_of_range_unreachable,
    "garbage_in_absent_slot": mut_garbage_in_absent_slot,
    "wrong_embedded_byte": mut_wrong_embedded_byte,
    "plain_indices_as_embedded": mut_plain_indices_as_embedded,
    "self_loop": mut_self_loop,
    "loop_to_ancestor": mut_loop_to_ancestor,
    "coarse_voxel": mut_coarse_voxel,
    "grid_halved": mut_grid_halved,
    "grid_doubled": mut_grid_doubled,
    "grid_2_22": mut_grid_2_22,
    "grid_garbage": mut_grid_garbage,
    "node_at_two_depths": mut_node_at_two_depths,
    "psum_reaches_count": mut_psum_reaches_count,
    "voxels_without_count": mut_voxels_without_count,
}


def mut_random_word(t, rng):
    """any one word of any node: a child word (voxel, index in or out of range, right or wrong byte), a mask byte or an nVoxelsPSum value; the
    model decides whether the result is legal"""
    nodes, nv, res, emb = t
    out = nodes.copy()
    i = int(rng.integers(0, len(out)))
    c = int(rng.integers(0, 8))
    what = int(rng.integers(0, 4))
    if what == 0:
        k = int(rng.integers(0, len(out) + 3))
        w = _word(k, out["mask"], emb) if k < len(out) else k
        if emb and rng.random() < 0.3:
            w = (w & IDX) | (int(rng.integers(0, 256)) << 24)
        out["children"][i, c] = LEAF if rng.random() < 0.25 else w
    elif what == 1:
        out["mask"][i] ^= np.uint8(1 << c)
    elif what == 2:
        out["psum"][i, c] = int(rng.choice([0, int(rng.integers(0, max(1, nv) + 2)), 2**32 - 1]))
    else:
        nv = int(rng.choice([0, max(0, nv - 1), nv + 1]))
    return out, nv, res, emb, None


def small_octree(O, rng, levels, dag, embedded, n_voxels=None):
    """a random voxel set of `levels` levels built by the oracle's port of the reference builder: (nodes, numberOfVoxels, gridRes, embedded)"""
    res = 1 << levels
    cells = res ** 3
    n = int(n_voxels if n_voxels is not None else rng.integers(1, min(cells, 40) + 1))
    if cells <= 1 << 20:
        codes = np.unique(rng.choice(cells, min(n, cells), replace=False).astype(np.uint64))
    else:
        codes = np.unique(rng.integers(0, cells, n, dtype=np.uint64))
    nodes = O.build_octree(codes, res, dag=dag, embed=embedded)
    return nodes, len(codes), res, embedded


# ---- voxel sets, their shapes, scenes and uploads ------------------------------------------------------------------------------------------------------------------
class Base:
    """a voxel set: sorted Morton codes, merged attributes, grid"""

    def __init__(self, name, morton, attrs, res, origin=(0.0, 0.0, 0.0), dps=None, he=None):
        self.name, self.morton, self.attrs, self.res = name, np.asarray(morton, np.uint64), np.asarray(attrs, np.uint8).reshape(-1, 8), res
        self.origin = np.asarray(origin, np.float32)
        self.dps = np.float32(1.0 / res) if dps is None else np.float32(dps)
        self.he = int((self.attrs[:, 4:7] != 0).any()) if he is None else he


def voxel_set(name, levels, n_cluster, n_scattered, seed):
    rng = np.random.default_rng(seed)
    res = 1 << levels
    box = max(2, res // 3)
    pts = np.concatenate([rng.integers(0, box, (n_cluster, 3)) + res // 4, rng.integers(0, res, (n_scattered, 3))])
    m = np.unique(D.morton(pts))
    attrs = rng.integers(0, 256, (len(m), 8), dtype=np.uint8)
    attrs[rng.random(len(m)) >= 0.1, 4:7] = 0
    attrs[:, 3] = 255
    return Base(name, m, attrs, res)


@pytest.fixture(scope="module")
def bases(O):
    tris = bunny_tris()
    cols, emis = position_colors(tris)
    b = O.build_scene_from_triangles(tris, 256, cols, emis)
    out = {"bunny256": Base("bunny256", b.morton, b.attrs, 256, b.origin, b.dps, b.has_emission),
           "random7": voxel_set("random7", 7, 20_000, 2_000, 7),
           "random9": voxel_set("random9", 9, 30_000, 3_000, 9)}
    for L in (1, 2, 3):
        rng = np.random.default_rng(100 + L)
        out["single%d" % L] = Base("single%d" % L, [int(rng.integers(0, 8 ** L))], [[200, 100, 50, 255, 0, 0, 0, 0]], 1 << L)
    s = D.DeepScene(14)
    sc = D.oracle_scene(O, s)
    out["deep14"] = Base("deep14", sc.morton, sc.attrs, s.res, s.origin, s.dps, sc.has_emission)
    return out


def shapes(O, base, emb, seed):
    """{shape: (nodes, keeps_builder_answers)}: every legal generator on the builder's octree of `base` (the empty octree: itself only)"""
    if base is None:
        empty = np.zeros(1, O.NODE_DTYPE)
        empty["children"] = LEAF
        return {"empty": (empty, True)}
    rng = np.random.default_rng(seed)
    nodes = O.build_octree(base.morton, base.res, dag=True, embed=emb)
    nv, res = len(base.morton), base.res
    out = {"builder": (nodes, True), "permute": (permute(nodes, emb, rng), True), "unreachable": (add_unreachable(nodes, emb, rng, 50, 50), True),
           "unshare": (unshare(nodes, emb), True), "empty_inner": (add_empty_inner(nodes, res, emb, rng, 64), False),
           "psum_zero": (psum_zero(nodes), False), "psum_random": (psum_random(permute(nodes, emb, rng), nv, res, rng), False)}
    if nv >= 2:
        out["psum_one_off"] = (psum_one_off(nodes, emb)[0], False)
    out["all"] = (permute(add_unreachable(add_empty_inner(unshare(nodes, emb), res, emb, rng), emb, rng), emb, rng), False)
    for k, (n, _) in out.items():
        set_masks_zero_padding(n)
        assert IntersectorOctreeGPU.check_upload(n, nv, res, emb) is None, k
    return out


def oracle_scene(O, base, nodes, emb):
    if base is None:
        return O.Scene(nodes, np.zeros((0, 8), np.uint8), (0.0, 0.0, 0.0), 0.25, 4, 0, embedded=emb)
    return O.Scene(nodes, base.attrs, base.origin, base.dps, base.res, base.he, embedded=emb)


def upload(mv, sc, emb, svo=None):
    svo = mv.IntersectorOctreeGPU() if svo is None else svo
    svo.upload(sc.nodes, sc.attrs, sc.origin, sc.dps, sc.grid_res, sc.has_emission, embeddedMask=emb)
    return svo
