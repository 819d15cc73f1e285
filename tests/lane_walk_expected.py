"""What the per-lane walk of include/mvrt/device.hpp (mvrt::DeviceOctree::walk<RANGE>) must give on the adversarial rays of tests/reference_pins.py, for
tests/test_lane_walk_cpu.py (the header built for the host, tests/cpp/lane_walk_host.cpp) and tests/test_gpu_lane_walk_edges.py (the same text on the MI355X):

  rays          R.rays_of (ties, origins on voxel corners / edges / faces, secondary-style origins, +-0, denormal, huge, +-inf and NaN direction components, the deep
                scenes' aimed rays) plus N_FAR far-origin rays (R.far_rays), plus -- deep scenes -- every ray the oracle "hits" at t = +inf twice more, with the
                limits MAX_FLOAT and +inf
  unlimited     the oracle's t, nMajor, vIndex, descents of the scene in the same flavour
  limited       the limit cycle of tests/test_gpu_range.py (limits / expected, moved here) around the oracle's unlimited t: the oracle's hit where t <= tMax, else a miss

Everything is computed once per (scene, flavour) and frozen."""
import os
import struct

import numpy as np

import deep_scenes as D
import reference_pins as R
from common import bunny_tris

f32 = np.float32
MAXF = f32(3.402823466e38)
CASES = ("t", "below", "above", "quarter", "four", "maxf", "inf", "zero", "minus", "nan")
OUTPUTS = ("t", "nMajor", "vIndex", "descents")
SCENES = ("bunny64", "random9", "deep14", "deep16")
# check_populations wants 1 000 oracle hits among the far rays at every k <= 8 and 500 at k = 23.  Hits thin out with k (at k = 23 an origin coordinate is rounded by
# about an extent): of 100 000 rays deep16 keeps 344 at k = 23 and deep14 395, of 160 000 they keep 633 and 714.
N_FAR = 160_000
MAGIC = 0x4B4C574C


def limits(sc, t_unlimited):
    """the per-ray limit: case i % 10 of CASES around the oracle's unlimited t of that ray (the scene's extent for a miss)"""
    ext = f32(f32(sc.dps) * f32(sc.grid_res))
    base = np.where(t_unlimited != MAXF, t_unlimited, ext).astype(f32)
    case = np.arange(len(base)) % len(CASES)
    with np.errstate(over="ignore"):
        choices = [base, np.nextafter(base, f32(0)), np.nextafter(base, f32(np.inf)), (f32(0.25) * base).astype(f32), (f32(4) * base).astype(f32),
                   np.full_like(base, MAXF), np.full_like(base, np.inf), np.zeros_like(base), np.full_like(base, -1), np.full_like(base, np.nan)]
    return np.choose(case, choices).astype(f32), case


def expected(want, sh, tmax):
    """the filtered oracle: its hit where t <= tMax in fp32 (false for a NaN limit), else the miss triple"""
    with np.errstate(invalid="ignore"):
        keep = (want["t"] != MAXF) & (want["t"] <= tmax)
    return {"t": np.where(keep, want["t"], MAXF).astype(np.float32), "nMajor": np.where(keep, want["nMajor"], -1).astype(np.int32),
            "vIndex": np.where(keep & (sh == 0), want["vIndex"], 0).astype(np.uint32)}, keep


_scenes = {}


def oracle_scene(O, name, embedded):
    """the oracle's Scene of a name of R.ray_scene in either flavour; plain = child words without masks (embed=False, flags 2)"""
    if embedded:
        return R.ray_scene(O, name).sc
    if (name, embedded) not in _scenes:
        rs = R.ray_scene(O, name)
        if name.startswith("bunny"):
            sc = O.build_scene_from_triangles(bunny_tris(), int(name[5:]), embed=False)
        elif name.startswith("random"):
            sc = O.Scene(O.build_octree(rs.morton, rs.sc.grid_res, embed=False), rs.sc.attrs, rs.sc.origin, rs.sc.dps, rs.sc.grid_res, embedded=False)
            sc.morton = rs.morton
        else:
            sc = D.oracle_scene(O, rs.deep, 2)
        lo, hi = sc.bounds()
        assert np.array_equal(lo, rs.lower) and np.array_equal(hi, rs.upper) and np.array_equal(sc.morton, rs.morton) and not sc.embedded
        _scenes[(name, embedded)] = sc
    return _scenes[(name, embedded)]


class Expectation:
    def __init__(self, O, name, embedded):
        self.name, self.embedded = name, embedded
        self.rs = R.ray_scene(O, name)
        self.sc = sc = oracle_scene(O, name, embedded)
        ro, rd, sh = R.rays_of(O, name)
        fro, frd, fsh, fk = R.far_rays_of(O, name, N_FAR)
        self.n_set = len(ro)  # [0, n_set): R.rays_of, [n_set, n_base): the far rays, [n_base, n): the t = +inf rays again
        ro, rd, sh = np.concatenate([ro, fro]), np.concatenate([rd, frd]), np.concatenate([sh, fsh])
        far_k = np.concatenate([np.full(self.n_set, -1, np.int32), fk])
        want = sc.trace(ro, rd, sh, threads=8, want_descents=True)
        want = {k: want[k] for k in OUTPUTS}
        tmax, case = limits(sc, want["t"])
        self.n_base = len(ro)
        inf = np.flatnonzero(np.isinf(want["t"]))
        again = np.concatenate([inf, inf])
        self.ro, self.rd, self.sh = np.concatenate([ro, ro[again]]), np.concatenate([rd, rd[again]]), np.concatenate([sh, sh[again]])
        self.far_k = np.concatenate([far_k, np.full(len(again), -1, np.int32)])
        self.want = {k: np.concatenate([v, v[again]]) for k, v in want.items()}
        self.tmax = np.concatenate([tmax, np.full(len(inf), MAXF, f32), np.full(len(inf), np.inf, f32)])
        self.case = np.concatenate([case, np.full(len(inf), CASES.index("maxf")), np.full(len(inf), CASES.index("inf"))])
        self.n_inf = len(inf)
        self.exp, self.keep = expected(self.want, self.sh, self.tmax)
        for a in (self.ro, self.rd, self.sh, self.far_k, self.tmax, self.case, self.keep, *self.want.values(), *self.exp.values()):
            a.setflags(write=False)

    def hits_in(self, case):
        return int(((self.want["t"] != MAXF) & (self.case == CASES.index(case))).sum())

    def check_populations(self):
        """no comparison of these rays is vacuous: enough hits in the limit cases a wrong cut gets wrong, at every distance, and at t = +inf; -> far hits per k"""
        hit = self.want["t"] != MAXF
        assert self.hits_in("t") >= 1000 and self.hits_in("below") >= 1000
        assert self.keep[hit & (self.case == CASES.index("t"))].all() and not self.keep[self.case == CASES.index("below")].any()
        per_k = np.bincount(self.far_k[hit & (self.far_k >= 0)], minlength=R.FAR_K)
        assert (per_k[:9] >= 1000).all() and per_k[23] >= 500, per_k
        if self.rs.deep is not None:
            # the reference's t = +inf "hits" of rays without a direction: by the first rule of the limit, t <= tMax, a miss under MAX_FLOAT, a hit under +inf
            assert self.n_inf >= 1
            tail = np.arange(self.n_base, len(self.ro))
            assert not self.keep[tail[:self.n_inf]].any() and self.keep[tail[self.n_inf:]].all() and np.isinf(self.exp["t"][tail[self.n_inf:]]).all()
        return per_k

    def check_unlimited(self, got, what):
        for k in OUTPUTS:
            same = R.bits(got[k]) == R.bits(self.want[k])
            assert same.all(), "%s, %s: %s differs from the oracle on %d of %d rays, first at %d" % (self.name, what, k, (~same).sum(), same.size, np.argmax(~same))

    def check_limited(self, got, what, occluded=True):
        """-> the descents the cut saved"""
        for k in ("t", "nMajor", "vIndex"):
            same = R.bits(got[k]) == R.bits(self.exp[k])
            assert same.all(), "%s, %s: limited %s differs from the filtered oracle on %d of %d rays, first at %d (limit case %s)" % (
                self.name, what, k, (~same).sum(), same.size, np.argmax(~same), CASES[self.case[np.argmax(~same)]])
        de, full = got["descents"], self.want["descents"]
        assert np.array_equal(de[self.keep], full[self.keep]), what  # an accepted hit walked exactly the unlimited walk
        assert (de <= full).all(), what
        for name in ("zero", "minus", "nan"):
            assert (de[self.case == CASES.index(name)] == 0).all(), (what, name)
        if occluded:
            # occluded() = the limited SHADOW ray of the same origin, direction and limit, whatever the ray's own flag
            assert np.array_equal(got["occluded"], self.keep.astype(np.uint8)), what
        return int(full.sum(dtype=np.uint64) - de.sum(dtype=np.uint64))


_expectations = {}


def expectation(O, name, embedded):
    if (name, embedded) not in _expectations:
        _expectations[(name, embedded)] = Expectation(O, name, embedded)
    return _expectations[(name, embedded)]


# ---- the input and output files of tests/cpp/lane_walk_host.cpp --------------------------------------------------------------------------------------
def node_lines(nodes, embedded):
    """(lines (n, 16) uint32, masks, psumCold) as the upload lays them out (csrc/kernels_setup.hip).  Embedded: children[8] with the child's mask
    in bits 24-31, then nVoxelsPSum[8].  Plain: children[8], the 8 child masks one byte each in two words (0 for a voxel or an absent child), six unused words;
    masks[node] = the node's own mask, psumCold[node * 8 + child] = nVoxelsPSum."""
    n = len(nodes)
    ch = np.ascontiguousarray(nodes["children"]).astype(np.uint32)
    lines = np.zeros((n, 16), np.uint32)
    lines[:, :8] = ch
    if embedded:
        lines[:, 8:] = nodes["psum"]
        return lines, None, None
    leaf = ch == 0xFFFFFFFF
    assert (ch[~leaf] < n).all()
    cm = np.where(leaf, 0, nodes["mask"][np.where(leaf, 0, ch)]).astype(np.uint32)
    for k in range(8):
        lines[:, 8 + k // 4] |= cm[:, k] << np.uint32(8 * (k % 4))
    return lines, np.ascontiguousarray(nodes["mask"], np.uint8), np.ascontiguousarray(nodes["psum"], np.uint32)


def write_input(path, exp, stack_mode, limited=True, rays=None):
    """the file tests/cpp/lane_walk_host.cpp reads, for the rays of an Expectation (or the index array `rays` of them)"""
    import massivevoxelraytracing_amd as mv
    sc, nodes = exp.sc, exp.sc.nodes
    v = mv.DeviceOctree()
    v.structBytes, v.flavour = 128, 0 if exp.embedded else 1
    v.lower[:], v.upper[:] = exp.rs.lower.tolist(), exp.rs.upper.tolist()
    v.dps, v.emissionScale, v.hasEmission = sc.dps, 1.0, sc.has_emission
    v.levels, v.numberOfNodes, v.numberOfVoxels = exp.rs.levels, len(nodes), len(sc.attrs)
    v.rootIndex, v.rootMask = len(nodes) - 1, int(nodes["mask"][-1])
    lines, masks, psum_cold = node_lines(nodes, exp.embedded)
    sel = slice(None) if rays is None else rays
    ro, rd, sh, tmax = exp.ro[sel], exp.rd[sel], exp.sh[sel], exp.tmax[sel]
    with open(path, "wb") as f:
        f.write(struct.pack("<4I2Q", MAGIC, stack_mode, int(limited), 0, len(nodes), len(ro)))
        f.write(bytes(v))
        f.write(lines.tobytes())
        if not exp.embedded:
            f.write(masks.tobytes())
            f.write(psum_cold.tobytes())
        for a, d in ((ro, f32), (rd, f32), (sh, np.uint8)) + (((tmax, f32),) if limited else ()):
            f.write(np.ascontiguousarray(a, d).tobytes())
    return len(ro)


def read_output(path, n, limited=True):
    """-> (unlimited outputs, limited outputs with `occluded` or None)"""
    raw = np.fromfile(path, np.uint8)
    assert len(raw) == n * (16 + (17 if limited else 0)), (len(raw), n)
    types = (np.float32, np.int32, np.uint32, np.uint32)
    four = lambda b: {k: raw[(b + i) * 4 * n:(b + i + 1) * 4 * n].view(d) for i, (k, d) in enumerate(zip(OUTPUTS, types))}
    if not limited:
        return four(0), None
    lim = four(4)
    lim["occluded"] = raw[32 * n:]
    return four(0), lim


LANE_WALK_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "lane_walk_host.cpp")
