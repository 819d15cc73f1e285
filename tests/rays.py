"""What the ray tests share: ray sets (random, tie, secondary-like, per-face occlusion rays), the comparison of hit records, uploads of oracle scenes, small scenes,
and the two user kernels on include/mvrt/device.hpp (tests/hip/device_api_probe.hip, tests/hip/range_probe.hip) compiled with hipcc and called through ctypes."""
import ctypes as C
import os
import subprocess
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
MAXF = np.float32(3.402823466e38)
OUTPUTS = ("t", "nMajor", "vIndex", "descents")
AXIS = np.array([1, 1, 2, 0, 2, 0])  # direction -> normal axis, in the order of mvrt.h: -Y +Y -Z +X +Z -X
PLUS = np.array([0, 1, 0, 1, 1, 0])


# ---- octrees and scenes --------------------------------------------------------------------------------------------------------------------------------------------
def upload(mv, sc, embedded=True):
    svo = mv.IntersectorOctreeGPU()
    svo.upload(sc.nodes, sc.attrs, sc.origin, sc.dps, sc.grid_res, sc.has_emission, embeddedMask=embedded)
    return svo


def make_pt(mv, O, sc, w, h, rgba, hw, hh, tile=(0, 1), hdri_scale=None):
    pt = mv.PathTracer()
    pt.setup(None)
    pt.set_tile(*tile)
    pt.resizeFrameBufferIfNeeded(None, w, h)
    pt.loadHDRIPixels(None, rgba, hw, hh, rgba, hw, hh)
    if hdri_scale is not None:
        pt.set_hdri_scale(hdri_scale)
    pt.m_intersectorOctreeGPU.upload(sc.nodes, sc.attrs, sc.origin, sc.dps, sc.grid_res, sc.has_emission)
    return pt


def voxel_scene(xyz, res):
    xyz = np.ascontiguousarray(xyz, np.uint32)
    attrs = np.full((len(xyz), 8), 255, np.uint8)
    attrs[:, 4:7] = 0
    return types.SimpleNamespace(xyz=xyz, attrs=attrs, res=res, origin=np.zeros(3, np.float32), dps=np.float32(1.0 / res))


def splitmix64(x):
    x = (x + np.uint64(0x9E3779B97F4A7C15)).astype(np.uint64)
    x = ((x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)).astype(np.uint64)
    x = ((x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)).astype(np.uint64)
    return x ^ (x >> np.uint64(31))


def synthetic_reference(O, res, n, seed):
    """numpy restatement of the documented generator (include/mvrt.h) + the oracle's merge and non-DAG build"""
    with np.errstate(over="ignore"):
        i = np.arange(n, dtype=np.uint64)
        h = splitmix64(np.uint64(seed) + i)
        c = splitmix64(h)
    m = np.uint64(res - 1)
    xyz = np.stack([h & m, (h >> np.uint64(21)) & m, (h >> np.uint64(42)) & m], -1).astype(np.uint32)
    morton = O.morton_encode_batch(xyz)
    rgb = (c & np.uint64(0xFFFFFF)) | np.uint64(0x404040)
    em = np.where((c >> np.uint64(56)) == 0, rgb, np.uint64(0))
    attrs = np.zeros((n, 8), np.uint8)
    for k in range(3):
        attrs[:, k] = ((rgb >> np.uint64(8 * k)) & np.uint64(255)).astype(np.uint8)
        attrs[:, 4 + k] = ((em >> np.uint64(8 * k)) & np.uint64(255)).astype(np.uint8)
    attrs[:, 3] = 255
    attrs[:, 7] = 255
    return O.merge_voxels(morton, attrs)


# ---- ray sets ------------------------------------------------------------------------------------------------------------------------------------------------------
def random_rays(sc, n, seed):
    """rays from around the grid onto random points of it, with axis-parallel / zero-component directions and rays from inside"""
    rng = np.random.default_rng(seed)
    lo, hi = sc.bounds()
    c = (lo + hi) / 2
    ext = (hi - lo).max()
    ro = (c + (rng.random((n, 3)) - 0.5) * ext * 2.5).astype(np.float32)
    tgt = (lo + rng.random((n, 3)) * (hi - lo)).astype(np.float32)
    rd = (tgt - ro).astype(np.float32)
    # a share of axis-parallel and zero-component directions (the 1/0 clamp path, voxCommon.hpp:265-269)
    k = n // 10
    rd[:k, 0] = 0.0
    rd[k:2 * k, 1] = 0.0
    rd[2 * k:3 * k, 2] = 0.0
    rd[3 * k:3 * k + 50] = np.array([0, 0, -1], np.float32)
    # rays starting inside the volume
    ro[4 * k:5 * k] = (lo + rng.random((k, 3)) * (hi - lo)).astype(np.float32)
    return ro, rd


def secondary_like_rays(sc, prim_ro, prim_rd, hits, seed):
    """rays that start ON the voxels other rays hit (what the path tracer's shadow / bounce rays are): origin = ro + rd * t as the shade kernel
    computes it, direction random; the hint = Morton code of the hit voxel"""
    rng = np.random.default_rng(seed)
    hit = hits["t"] != np.float32(3.402823466e38)
    t = hits["t"][hit].astype(np.float32)
    ro = (prim_ro[hit] + prim_rd[hit] * t[:, None]).astype(np.float32)
    rd = rng.normal(size=ro.shape).astype(np.float32)
    hint = sc.morton[hits["vIndex"][hit]].astype(np.uint64)
    return ro, rd, hint


def tie_rays(sc, n_out=3000, n_in=1500, seed=3):
    """diagonals through lattice points of the octree from dyadic distances, and from ON the lattice planes"""
    lo, _ = sc.bounds()
    ext = np.float32(sc.dps * sc.grid_res)
    levels = int(np.log2(sc.grid_res))
    rng = np.random.default_rng(seed)
    dirs = [(1, 1, 1), (1, 1, -1), (1, -1, 1), (-1, 1, 1), (1, 1, 0.5), (1, 0.5, 1), (0.5, 1, 1), (1, 0.5, 0.25), (2, 1, 1), (1, 2, -1), (-1, -1, -1), (1, -1, -0.5)]
    ros, rds = [], []
    for k in range(n_out):
        lvl = int(rng.integers(1, levels + 1))
        cell = ext / np.float32(2 ** lvl)
        p = lo + cell * rng.integers(0, 2 ** lvl + 1, size=3).astype(np.float32)
        d = np.array(dirs[k % len(dirs)], np.float32)
        s = np.float32(2 ** int(rng.integers(0, 3)))
        ros.append((p - d * ext * s).astype(np.float32))
        rds.append(d if k % 3 else d * np.float32(0.5))
    for k in range(n_in):
        lvl = int(rng.integers(1, levels + 1))
        cell = ext / np.float32(2 ** lvl)
        ros.append((lo + cell * rng.integers(0, 2 ** lvl + 1, size=3).astype(np.float32)).astype(np.float32))
        rds.append(np.array(dirs[k % len(dirs)], np.float32))
    return np.array(ros, np.float32), np.array(rds, np.float32)


def ray_set(sc, n, seed):
    ro, rd = random_rays(sc, n, seed)
    tr, td = tie_rays(sc)
    ro, rd = np.concatenate([ro, tr]), np.concatenate([rd, td])
    sh = (np.random.default_rng(seed + 1).random(len(ro)) < 0.3).astype(np.uint8)
    return ro, rd, sh


def face_origins(xyz, face_voxel, face_dir, lower, dps):
    """ro[a] = lower[a] + (float)c2 * (0.5f * dps), c2 in half voxels: the voxel's middle in the plane, the face on the normal axis"""
    f32 = np.float32
    c2 = 2 * xyz[face_voxel].astype(np.int64) + 1
    c2[np.arange(len(c2)), AXIS[face_dir]] += np.where(PLUS[face_dir] == 1, 1, -1)
    h = f32(f32(0.5) * f32(dps))
    return (np.asarray(lower, f32)[None, :] + (c2.astype(f32) * h).astype(f32)).astype(f32)


def oracle_t(mv, sc, xyz, face_voxel, face_dir, K):
    """the oracle's unlimited t of the K occlusion rays of every face: (nFaces, K)"""
    lo, _ = sc.bounds()
    ro = face_origins(xyz, face_voxel, face_dir, lo, np.float32(sc.dps))
    dirs = mv.ao_directions(K)
    rd = dirs[face_dir]  # (n, K, 3)
    ro = np.ascontiguousarray(np.broadcast_to(ro[:, None, :], rd.shape)).reshape(-1, 3)
    t = sc.trace(ro, rd.reshape(-1, 3), np.ones(len(ro), np.uint8), threads=8)["t"]
    return t.reshape(len(face_voxel), K)


def expected_open(t, radius):
    return (~((t != MAXF) & (t <= np.float32(radius)))).sum(1).astype(np.uint16)


# ---- hit records ---------------------------------------------------------------------------------------------------------------------------------------------------
def assert_hits_equal(a, b):
    assert np.array_equal(a["t"], b["t"]), "t"
    hit = a["t"] != np.float32(3.402823466e38)
    assert np.array_equal(a["nMajor"][hit], b["nMajor"][hit]), "nMajor of the hits"
    assert np.array_equal(a["vIndex"][hit], b["vIndex"][hit]), "vIndex of the hits"
    assert (b["nMajor"][~hit] == -1).all(), "nMajor of the misses"
    if "descents" in a and "descents" in b:
        assert np.array_equal(a["descents"], b["descents"]), "descents"


# ---- the user kernels ----------------------------------------------------------------------------------------------------------------------------------------------
def compile_probe(out_dir, flags):
    so = os.path.join(str(out_dir), "device_api_probe%s.so" % "".join(flags).replace("=", "_"))
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror"] + flags +
                          ["-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "hip", "device_api_probe.hip"), "-o", so], timeout=300)
    lib = C.CDLL(so)
    lib.probe_trace.restype = C.c_int
    lib.probe_trace.argtypes = [C.c_void_p, C.c_uint64] + [C.c_void_p] * 11 + [C.c_int]
    lib.probe_attrs.restype = C.c_int
    lib.probe_attrs.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 4
    lib.probe_camera.restype = C.c_int
    lib.probe_camera.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    return lib


def probe_trace(mv, probe, view, ro, rd, sh=None, mode=0):
    ro = np.ascontiguousarray(ro, np.float32).reshape(-1, 3)
    rd = np.ascontiguousarray(rd, np.float32).reshape(-1, 3)
    n = len(ro)
    if n == 0:
        assert probe.probe_trace(C.byref(view), 0, *([None] * 11), mode) == 0
        return {k: np.zeros(0, d) for k, d in (("t", np.float32), ("nMajor", np.int32), ("vIndex", np.uint32), ("descents", np.uint32))}
    dev = [mv.DeviceArray.from_host(np.ascontiguousarray(a)) for a in (ro[:, 0], ro[:, 1], ro[:, 2], rd[:, 0], rd[:, 1], rd[:, 2])]
    dsh = None if sh is None else mv.DeviceArray.from_host(np.ascontiguousarray(sh, np.uint8))
    out = [mv.DeviceArray(n, d) for d in (np.float32, np.int32, np.uint32, np.uint32)]
    rc = probe.probe_trace(C.byref(view), n, *[a.ptr for a in dev], None if dsh is None else dsh.ptr, *[a.ptr for a in out], mode)
    assert rc == 0, rc
    return dict(zip(("t", "nMajor", "vIndex", "descents"), (a.to_host() for a in out)))


def compile_range_probe(out_dir, flags):
    so = os.path.join(str(out_dir), "range_probe%s.so" % "".join(flags).replace("=", "_"))
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror"] + flags +
                          ["-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "hip", "range_probe.hip"), "-o", so], timeout=300)
    lib = C.CDLL(so)
    lib.probe_range.restype = C.c_int
    lib.probe_range.argtypes = [C.c_void_p, C.c_uint64] + [C.c_void_p] * 13 + [C.c_int]
    return lib


def probe_range(mv, probe, view, ro, rd, sh, tmax, mode):
    n = len(ro)
    dev = [mv.DeviceArray.from_host(np.ascontiguousarray(a)) for a in (ro[:, 0], ro[:, 1], ro[:, 2], rd[:, 0], rd[:, 1], rd[:, 2])]
    dsh, dlim = mv.DeviceArray.from_host(np.ascontiguousarray(sh, np.uint8)), mv.DeviceArray.from_host(np.ascontiguousarray(tmax, np.float32))
    out = [mv.DeviceArray(n, d) for d in (np.float32, np.int32, np.uint32, np.uint32, np.uint8)]
    rc = probe.probe_range(C.byref(view), n, *[a.ptr for a in dev], dsh.ptr, dlim.ptr, *[a.ptr for a in out], mode)
    assert rc == 0, rc
    return dict(zip(OUTPUTS + ("occluded",), (a.to_host() for a in out)))
