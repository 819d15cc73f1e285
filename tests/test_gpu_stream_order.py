"""Every entry point of include/mvrt.h that takes a `stream`, made on a NON-BLOCKING stream S that is held back, and with the default stream held back.

The C++ usage programs and the other GPU tests pass the default stream or a blocking one, which waits for the default stream by itself: a kernel, memset, copy or
hipcub call the library issues on stream 0 instead of the caller's stream gives the right answer there.  Here it does not.  One table (CASES), three regimes a case:

  A  S held (streams.Held): behind the hold the real inputs are copied over the decoy on S (mvrt_memcpy_d2d), the call is made on S, the outputs are copied out on S
     and only S is waited for.  What the library reads too early, or on another stream, is the decoy: a valid input whose result differs.
  B  the default stream held, the same on S.  What the library issues on the default stream without joining it back into S runs late.
  C  the harness checks itself: A with the call made on the default stream while its producer waits behind the hold on S.  The result has to be the decoy's (at
     least not the real one): otherwise the hold did not outlast the call and A proves nothing for that case.  Cases whose inputs are host arrays have no C.

Decoys are valid inputs by construction (another ray set, another in-grid voxel list, another mask): a mis-ordered read gives a wrong answer, never a fault.
Expected values: where the operator's CPU model in tests/*_expected.py is a call or two away (`cpu`), the un-held result on the default stream is held to it
here, and tests/test_stream_order_cpu.py asserts on the CPU that the model's answers for the real and the decoy inputs differ.  The other cases say in `no_model`
why theirs is further away (hits and frames of the oracle); for those, and for the trace half of the in-place cases, the expectation is the library's own
un-held result, which the test named in `pinned` holds to its reference, and real != decoy is asserted on those results before any stream is held.

WHAT A HOLD COVERS.  A hold covers a call up to the first point where the library itself waits for the held stream; regime B covers it up to the first wait for the
default stream or the device (a synchronous hipMemcpy / hipMemset, the hipFree of scratch, which waits for the whole device, hipDeviceSynchronize).  The internal
waits, found by reading the sources:
  - no wait at all, covered whole by A and B: trace_batch, trace_batch_hinted (api.hip traceBatch: a launch), trace_batch_range / _cone, resolve_buffer,
    assemble_tiles, denoise_buffers with the caller's scratch, memcpy_d2d.  The path tracer's pt_step / step_matrices / join / resolve / clear_framebuffer queue
    on `stream` and the slot streams and return; their cases set the tracer up BEFORE the window, so the first step and what follows it up to the first
    read-back wait behind the hold.  render_primary(_lod) launch and return too, but their cases rebuild the octree in the same window first (next but one
    item), so the render itself runs with the hold over.
  - one wait for `stream` at their end, because scratch or a host count is released or returned there, covered whole by A, and by B up to that hipFree:
    compact_indices (api.hip), pt_error_mask (the count).
  - a validation or count pass, hipStreamSynchronize( stream ), then the work: surface_ao (kernels_range.hip: kAoValidate, the wait, kSurfaceAo),
    pt_set_sample_mask (the active list, the wait, the drain), the masked surface calls and surface_smooth (their face count comes back through the scan's
    wait, voxel_passes.h) and the nearest queries (kernels_nearest.hip, kernels_query.hip: a wait per pass for its scratch).  A covers the pass that reads
    the caller's arrays first; what follows the wait runs with the hold over.  A launch of the second half moved to stream 0 is therefore NOT seen: the scratch's
    hipFree on return waits for it (tried with kSurfaceAo on stream 0: all three regimes pass; with kResolve on stream 0 regime A fails with the decoy's image).
  - every listing with a host count, every voxel-list build, edit and in-place operator: encodeVoxels (svo_build.hip) and the first hipcub call (devbuf.h
    withCubTemp) end in hipStreamSynchronize( stream ), adoptBuild (api.hip) in hipDeviceSynchronize.  A covers the reads of the caller's arrays up to that first
    wait, B up to the first hipFree; the trace and the walk that follow in the same window run with the hold over.
  - pt_setup, pt_load_hdri(_file), pt_update_scene and a reallocating resize end in a wait for `stream` and free scratch: in pt_setup_to_first_frame, the one case
    that makes them in the window, pt_setup's wait uses the hold up (A), load_hdri's synchronous copy of the totals does (B), and the calls after it are
    unheld.  read_framebuffer / read_aov / read_moments / read_denoised and get_stats end in a wait for `stream`, since they return host data; pt_denoise has no
    wait of its own, pt_error_mask one at its end, to_image_async none (its caller waits).  Each of them has a case of its own in which it is the first call
    after the steps that waits, so the steps, the call and its read-back are all behind the hold."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import voxel_sets as VS
from common import GOLDEN, bunny_tris, position_colors, probe_camera
from streams import streams  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

RES, N_VOXELS, N_RAYS, CAP = 16, 400, 4096, 6 * 16 ** 3  # CAP: no listing of a 16^3 grid is longer (six faces a cell)
W, H, STEPS = 17, 13, 2
u8, u16, u32, u64, i32, f32 = np.uint8, np.uint16, np.uint32, np.uint64, np.int32, np.float32


# ---- inputs, made on the CPU ------------------------------------------------------------------------------------------------------------------------------------
def voxel_set(seed, shell_at, block_at):
    """(xyz (N_VOXELS, 3) uint32 distinct cells of the 16^3 grid, attribs): a hollow 6^3 shell (an enclosed region), a solid 4^3 block (an erosion leaves
    something) and single voxels (small components) up to N_VOXELS"""
    rng = np.random.default_rng(seed)
    g = np.zeros((RES,) * 3, bool)
    s = VS.shell(shell_at, shell_at + 6)
    g[s[:, 0], s[:, 1], s[:, 2]] = True
    b = block_at
    g[b:b + 4, b:b + 4, b:b + 4] = True
    free = np.argwhere(~g)
    extra = free[rng.permutation(len(free))[: N_VOXELS - int(g.sum())]]
    g[extra[:, 0], extra[:, 1], extra[:, 2]] = True
    xyz = np.argwhere(g).astype(u32)
    xyz = xyz[rng.permutation(len(xyz))]
    assert len(xyz) == N_VOXELS and xyz.max() < RES
    at = VS.colours(N_VOXELS, seed)
    at[:, 3] = at[:, 7] = 255
    return xyz, at


SET1, SET2, SET3 = voxel_set(1, 1, 10), voxel_set(2, 8, 2), voxel_set(3, 5, 0)
EXTENT = f32(VS.DPS * RES)


def ray_set(seed):
    """SoA rays onto the grid from around it and from inside, shadow flags, limits, cones: 7 + 1 + 2 arrays"""
    rng = np.random.default_rng(seed)
    c = VS.LOWER + EXTENT / 2
    d = rng.normal(size=(N_RAYS, 3))
    ro = c + d / np.linalg.norm(d, axis=1)[:, None] * EXTENT * 1.5
    ro[: N_RAYS // 8] = VS.LOWER + rng.random((N_RAYS // 8, 3)) * EXTENT
    tgt = VS.LOWER + rng.random((N_RAYS, 3)) * EXTENT
    ro, rd = ro.astype(f32), (tgt - ro).astype(f32)
    sh = (rng.random(N_RAYS) < 0.3).astype(u8)
    tmax = (rng.random(N_RAYS) * 1.5).astype(f32)
    cone_a, cone_b = (rng.random(N_RAYS) * VS.DPS).astype(f32), (rng.random(N_RAYS) * 0.2).astype(f32)
    return [np.ascontiguousarray(a) for a in (ro[:, 0], ro[:, 1], ro[:, 2], rd[:, 0], rd[:, 1], rd[:, 2], sh, tmax, cone_a, cone_b)]


RAYS, DECOY_RAYS = ray_set(11), ray_set(12)


def morton(xyz):
    import surface_expected as SX
    return SX.morton(np.asarray(xyz, np.int64)).astype(u64)


def hints(seed):
    """per ray the code of some voxel of SET1 (any existing voxel is a valid hint for any ray) or ~0"""
    rng = np.random.default_rng(seed)
    h = morton(SET1[0])[rng.integers(0, N_VOXELS, N_RAYS)]
    h[rng.random(N_RAYS) < 0.2] = u64(0xFFFFFFFFFFFFFFFF)
    return h


def triangles(flip):
    """the bunny inside the grid of the voxel sets (`flip`: mirrored in x, the decoy) -> (vertices, colours, emissions) (n, 3) each"""
    t = bunny_tris()[::7]
    cols, emis = position_colors(t)
    v = t.reshape(-1, 3).astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    n = (v - lo) / (hi - lo).max()
    if flip:
        n[:, 0] = n[:, 0].max() - n[:, 0]
    return (VS.LOWER + n * float(EXTENT) * 0.97 + 0.01 * float(EXTENT)).astype(f32), cols.reshape(-1, 3), emis.reshape(-1, 3)


def camera(decoy):
    return probe_camera(VS.LOWER, VS.DPS, RES, focus=0.5, lens_r=0.002, offset=(0.1, 0.35, 0.4) if decoy else (0.4, 0.25, 0.35))


def look_at(decoy):
    """(view, proj) column-major, as GetCameraMatrix gives them"""
    cam = camera(decoy)
    o, front, up, right = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    view = np.eye(4, dtype=f32)
    view[0, :3], view[1, :3], view[2, :3] = right, up, -front
    view[:3, 3] = -view[:3, :3] @ o
    fl = 1.0 / float(cam[12])
    proj = np.zeros((4, 4), f32)
    proj[0, 0], proj[1, 1], proj[2, 2], proj[2, 3], proj[3, 2] = fl / (W / H), fl, -1.002, -0.2, -1.0
    return np.ascontiguousarray(view.T).reshape(16), np.ascontiguousarray(proj.T).reshape(16)


def sample_mask(decoy, n):
    m = np.ones(n, u8) if decoy else (np.random.default_rng(5).random(n) < 0.5).astype(u8)
    m[W * H:] = 0  # the padding of the last tile is never sampled
    return m


def denoise_frame(seed):
    import denoise_cases as DC
    return [np.array(b) for b in DC.assemble(DC.fields(W, H, seed))]


def frame_f32(seed, n):
    return (np.random.default_rng(seed).random((n, 4)) * 3).astype(f32)


# ---- the table --------------------------------------------------------------------------------------------------------------------------------------------------
class Case:
    """name; apis: the mvrt_* entry points the case makes on the stream under test; make( world ) -> a Run; device_inputs: False = host inputs only, no regime C;
    pinned: the test that holds the un-held result to its CPU reference; cpu( which ) -> the CPU model's answer for the real (0) / decoy (1) inputs, anything
    `same` compares: a list aligned with the outputs, None where the model says nothing; no_model: why a case without `cpu` has none (the model is more than a
    call or two away)"""

    def __init__(self, name, apis, make, device_inputs=True, pinned="", cpu=None, no_model=""):
        self.name, self.apis, self.make, self.device_inputs, self.pinned, self.cpu, self.no_model = name, tuple(apis), make, device_inputs, pinned, cpu, no_model


class Run:
    """inputs: [(device array, real host, decoy host)]; outputs: device arrays, zeroed before every regime and copied out on the stream afterwards;
    prepare(): un-held, puts handles into the decoy state; call( stream, which ) -> further host results (counts); check( host results ): the CPU model"""
    inputs, outputs, check = (), (), None

    def prepare(self):
        pass


CASES = []
# host time of every case's whole call on the default stream, nothing held (the second, "decoy", has its code loaded): printed when the module is done, it
# re-measures streams.MEASURED_CALL_MS, which the hold is derived from; nothing is asserted on it
CALL_MS = {"real": [], "decoy": []}


def case(name, apis, **kw):
    def deco(make):
        CASES.append(Case(name, apis, make, **kw))
        return make
    return deco


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def agrees(got, model):
    """the un-held result against the CPU model: every output the model speaks of (an array each) holds the model's entries, and behind them the zeros it was
    cleared to, so the length the library wrote is the model's too.  The host counts a call returns are not part of a model: they are compared between the
    regimes only"""
    assert len(model) <= len(got) and all(m is None or np.ndim(m) >= 1 for m in model), "a model lists arrays, aligned with the outputs"
    return all(m is None or (np.array_equal(np.asarray(g)[: len(m)], m) and not np.asarray(g)[len(m):].any()) for g, m in zip(got, model))


def stated(model):
    return [m for m in model if m is not None]


ORACLE = "the expected hits are the oracle's: a scene built from the voxels, then its trace, then the comparison of hit records (rays.assert_hits_equal)"
FRAME = "the expected frame is the oracle's path tracer on an oracle scene with the decoded map: test_gpu_parity.test_path_tracer_bit_exact takes a dozen lines"


def differing(a, b):
    return sum(int(np.count_nonzero(np.asarray(x) != np.asarray(y))) if np.shape(x) == np.shape(y) else max(np.size(x), np.size(y)) for x, y in zip(a, b))


def total(a):
    return sum(int(np.size(x)) for x in a)


class World:
    """what the cases share: the package, the stream helper, device copies made once"""

    def __init__(self, st):
        self.st, self.mv = st, st.mv
        mv = self.mv
        self.keep = []  # device arrays and handles that must not be freed inside a held window (hipFree waits for the whole device)
        self.svo1 = VS.build(mv, SET1[0], RES, attribs=SET1[1])  # the fixed octree of group 1
        self.svo1.lod_prepare()
        self.other = VS.build(mv, SET3[0], RES, attribs=SET3[1])  # the second operand of combine, nearest_between, transfer_attributes
        self.rays = [mv.DeviceArray.from_host(a) for a in RAYS[:7]]  # the fixed rays of the in-place cases
        rgba, self.hw, self.hh = mv.read_rgbe_file(os.path.join(GOLDEN, "monks_forest_s.hdr"))
        self.rgba = rgba
        self.tris = [triangles(False), triangles(True)]

    def dev(self, a):
        return self.mv.DeviceArray.from_host(np.ascontiguousarray(a))

    def out(self, shape, dtype):
        return self.mv.DeviceArray(shape, dtype)

    def tmp(self, shape, dtype):
        """a device array made inside a held window: kept until the window is over"""
        self.keep.append(self.mv.DeviceArray(shape, dtype))
        return self.keep[-1]

    def trace(self, svo, outs, stream):
        svo.intersect_device(N_RAYS, *self.rays, *outs, None, stream)


def trace_outs(w):
    return [w.out(N_RAYS, f32), w.out(N_RAYS, i32), w.out(N_RAYS, u32)]


# ---- 1. device in, device out -----------------------------------------------------------------------------------------------------------------------------------
def ray_case(name, api, picks, extra_in, outs, call, pinned):
    """picks: indices into ray_set() of the arrays the call takes; extra_in: further (real, decoy) host inputs"""
    @case(name, [api], pinned=pinned, no_model=ORACLE)
    def make(w):
        r = Run()
        r.inputs = [(w.dev(DECOY_RAYS[k]), RAYS[k], DECOY_RAYS[k]) for k in picks] + [(w.dev(d), a, d) for a, d in extra_in()]
        r.outputs = [w.out((N_RAYS,) + s, d) for s, d in outs]
        r.call = lambda stream, which: call(w, [i[0] for i in r.inputs], r.outputs, stream)
        return r


def _lib_call(w, fn, *args):
    rc = getattr(w.mv.lib(), fn)(*args)
    assert rc == 0, w.mv.lib().mvrt_last_error()


HIT = [((), f32), ((), i32), ((), u32), ((), u32)]
ray_case("trace_batch", "mvrt_trace_batch", range(7), lambda: [], HIT, lambda w, i, o, s: w.svo1.intersect_device(N_RAYS, *i, *o, s),
         "test_gpu_parity.py::test_trace_batch_bit_exact")
ray_case("trace_batch_hinted", "mvrt_trace_batch_hinted", range(7), lambda: [(hints(1), hints(2))], HIT,
         lambda w, i, o, s: _lib_call(w, "mvrt_trace_batch_hinted", w.svo1._h, N_RAYS, *[a.ptr for a in i], *[a.ptr for a in o], s),
         "test_gpu_parity.py::test_start_below_the_root_gives_the_results_of_the_walk_from_the_root")
ray_case("trace_batch_range", "mvrt_trace_batch_range", range(8), lambda: [], HIT, lambda w, i, o, s: w.svo1.intersect_range_device(N_RAYS, *i, *o, s),
         "test_gpu_range.py")
ray_case("trace_batch_cone", "mvrt_trace_batch_cone", (0, 1, 2, 3, 4, 5, 8, 9), lambda: [],
         [((), f32), ((), i32), ((), u32), ((), u64), ((), u32), ((8,), u8), ((), u32)], lambda w, i, o, s: w.svo1.intersect_cone_device(N_RAYS, *i, *o, s),
         "test_gpu_cone.py::test_cone_rays_equal_the_model")


def handle_inputs(w):
    """the voxel list a case builds its handle from behind the hold: SET2 over the decoy SET1"""
    return [(w.dev(SET1[0]), SET2[0], SET1[0]), (w.dev(SET1[1]), SET2[1], SET1[1])]


def build_from(w, svo, ins, stream, edit=False):
    if edit:
        svo.edit_voxels(ins[0], ins[1], None, stream)
    else:
        svo.build_voxels(ins[0], ins[1], origin=VS.LOWER, dps=VS.DPS, gridRes=RES, stream=stream)


def render_case(name, api, lod):
    """the camera is a host argument: the device input is the octree, rebuilt from the list behind the hold"""
    @case(name, [api, "mvrt_svo_build_voxels"] + (["mvrt_svo_lod_prepare"] if lod else []),
          pinned="test_gpu_cone.py::test_render_lod" if lod else "test_gpu_parity.py::test_render_primary_golden_and_oracle", no_model=ORACLE)
    def make(w):
        r = Run()
        svo = w.mv.IntersectorOctreeGPU()
        r.inputs = handle_inputs(w)
        n = W * H
        r.outputs = [w.out((n, 4), u8), w.out(n, f32), w.out(n, i32), w.out(n, u32), w.out(n, u32)]
        r.prepare = lambda: build_from(w, svo, [w.dev(SET1[0]), w.dev(SET1[1])], None)
        cam = camera(False)

        def call(stream, which):
            build_from(w, svo, [i[0] for i in r.inputs], stream)
            if lod:
                svo.lod_prepare(stream)
                _lib_call(w, api, svo._h, cam.ctypes.data_as(C.c_void_p), W, H, 1.5, 1, *[o.ptr for o in r.outputs], stream)
            else:
                _lib_call(w, api, svo._h, cam.ctypes.data_as(C.c_void_p), W, H, 1, *[o.ptr for o in r.outputs], stream)
        r.call = call
        return r


render_case("render_primary", "mvrt_render_primary", False)
render_case("render_primary_lod", "mvrt_render_primary_lod", True)


def buffer_case(name, api, ins, outs, call, pinned, cpu=None, no_model=""):
    @case(name, [api], pinned=pinned, cpu=cpu, no_model=no_model)
    def make(w):
        r = Run()
        pairs = ins()
        r.inputs = [(w.dev(d), a, d) for a, d in pairs]
        r.outputs = [w.out(s, d) for s, d in outs]
        r.call = lambda stream, which: call(w, [i[0] for i in r.inputs], r.outputs, stream)
        if cpu:
            r.check = lambda got: agrees(got, cpu(0))
        return r


N_FLAGS = 70001  # more than one scan tile of 256 * 256 flags


def flags(decoy):
    return (np.random.default_rng(21 + decoy).random(N_FLAGS) < 0.4).astype(u8)


def compact_cpu(which):
    keep = flags(which)
    incl = np.cumsum(keep, dtype=np.uint64)
    return [np.where(keep != 0, incl - 1, 0xFFFFFFFF).astype(u32), np.array([incl[-1]], u32)]


buffer_case("compact_indices", "mvrt_compact_indices", lambda: [(flags(0), flags(1))], [(N_FLAGS, u32), (1, u32)],
            lambda w, i, o, s: _lib_call(w, "mvrt_compact_indices", i[0].ptr, N_FLAGS, o[0].ptr, o[1].ptr, s), "test_gpu_parity.py::test_compaction_indices_bit_exact",
            cpu=compact_cpu)
buffer_case("memcpy_d2d", "mvrt_memcpy_d2d", lambda: [(frame_f32(1, 999), frame_f32(2, 999))], [((999, 4), f32)],
            lambda w, i, o, s: w.mv.memcpy_d2d(o[0], i[0], o[0].nbytes, s), "the copy itself", cpu=lambda which: [frame_f32(1 + which, 999)])
buffer_case("resolve_buffer", "mvrt_resolve_buffer", lambda: [(frame_f32(3, W * H), frame_f32(4, W * H))], [((W * H, 4), u8)],
            lambda w, i, o, s: w.mv.resolve_buffer(i[0], W * H, o[0], s), "test_gpu_denoise_synthetic.py (resolve)",
            no_model="the resolve's rounding is the oracle's (denoise_cases.resolve_ordinary, O.resolve): not a model of tests/")


def _denoise(w, i, o, s):
    nbytes = w.mv.denoise_scratch_bytes(W, H)
    if not hasattr(w, "denoise_scratch"):
        w.denoise_scratch = w.out(nbytes, u8)
    w.mv.denoise_buffers(*i, W, H, o[0], w.denoise_scratch, nbytes, s, iterations=3)


buffer_case("denoise_buffers", "mvrt_denoise_buffers", lambda: list(zip(denoise_frame(101), denoise_frame(102))), [((W * H, 4), f32)], _denoise,
            "test_gpu_denoise_synthetic.py", no_model="denoise_expected.denoise needs the oracle's exp and takes seconds a frame")
TILE_STRIDE = 256  # owned pixels of a rank: 221 pixels in tiles of MVRT_TILE_PIXELS, two ranks
buffer_case("assemble_tiles", "mvrt_pt_assemble_tiles", lambda: [(frame_f32(5, 2 * TILE_STRIDE), frame_f32(6, 2 * TILE_STRIDE))], [((W * H, 4), f32)],
            lambda w, i, o, s: w.mv.assemble_tiles(i[0], 2, TILE_STRIDE, W, H, o[0], s), "test_gpu_adaptive.py (assembled frame buffer)",
            cpu=lambda which: [frame_f32(5 + which, 2 * TILE_STRIDE)[: W * H]])  # (221 pixels: block 0 alone, rank 0's first pixels)


def faces_of(xyz):
    """(faceVoxel, faceDir) of the first 600 exposed faces of a set: valid faces of SET1's octree when made from SET1"""
    import surface_expected as SX
    v = SX.sorted_voxels(xyz)
    fv, fd = SX.faces(v, SX.masks_of(v, RES))[:2]
    return np.ascontiguousarray(fv[:600], u32), np.ascontiguousarray(fd[:600], u8)


def ao_inputs():
    fv, fd = faces_of(SET1[0])
    return [(fv, np.ascontiguousarray(fv[::-1])), (fd, np.ascontiguousarray(fd[::-1]))]  # the decoy: the same valid faces in reverse order


buffer_case("surface_ao", "mvrt_svo_surface_ao", ao_inputs, [(600, u16)],
            lambda w, i, o, s: w.svo1.surface_ao_device(600, i[0], i[1], 16, 4 * VS.DPS, o[0], s), "test_gpu_ao.py::test_bunny_32", no_model=ORACLE)


def masks(decoy):
    """caller-supplied face masks of SET1's voxels: any six bits a voxel are valid"""
    return np.random.default_rng(31 + decoy).integers(0, 64, N_VOXELS).astype(u8)


def masked_faces(which, weld):
    """the faces of SET1's voxels under the caller's masks: surface_expected.faces, then positions or the weld"""
    import surface_expected as SX
    fv, fd, corners = SX.faces(SX.sorted_voxels(SET1[0]), masks(which))
    if not weld:
        return [fv, fd, SX.positions(corners, VS.LOWER, VS.DPS)]
    vertices, indices = SX.weld(corners, RES, VS.LOWER, VS.DPS)
    return [fv, fd, indices, vertices]


def smooth_cpu(which):
    import smooth_expected as SM
    r = SM.smooth(SET1[0], RES, VS.LOWER, VS.DPS, 4, (256, 256), 127, masks=masks(which))
    return [r[k] for k in ("faceVoxel", "faceDir", "indices", "vertices", "displacements", "neighbours")]


def smooth_params(w):
    p = w.mv.SmoothParams()
    _lib_call(w, "mvrt_smooth_default_params", C.byref(p))
    p.iterations, p.weightEven, p.weightOdd, p.limit = 4, 256, 256, 127
    return p


def masked_case(name, api, outs, call, **kw):
    buffer_case(name, api, lambda: [(masks(0), masks(1))], outs, call, "test_gpu_exterior.py (caller-supplied masks)", **kw)


def _counts(out):
    return [np.array(out if isinstance(out, tuple) else (out,), u64)]


masked_case("surface_quads_masked", "mvrt_svo_surface_quads_masked", [(CAP, u32), (CAP, u8), ((CAP, 4, 3), f32)],
            lambda w, i, o, s: _counts(w.svo1.surface_quads_device(CAP, *o, s, masks=i[0])), cpu=lambda which: masked_faces(which, False))
masked_case("surface_mesh_masked", "mvrt_svo_surface_mesh_masked", [(CAP, u32), (CAP, u8), ((CAP, 4), u32), ((CAP, 3), f32)],
            lambda w, i, o, s: _counts(w.svo1.surface_mesh_device(CAP, CAP, *o, s, masks=i[0])), cpu=lambda which: masked_faces(which, True))
masked_case("surface_merged_masked", "mvrt_svo_surface_merged_masked", [(CAP, u32), (CAP, u8), ((CAP, 2), u32), ((CAP, 4, 3), f32), ((CAP, 4), u32), ((CAP, 3), f32)],
            lambda w, i, o, s: _counts(w.svo1.surface_merged_device(3, CAP, CAP, *o, s, masks=i[0])),
            no_model="merge_expected.merged computes the exposure masks itself and takes none: the masked form is its body restated")
buffer_case("surface_smooth", "mvrt_svo_surface_smooth", lambda: [(masks(0), masks(1))],
            [(CAP, u32), (CAP, u8), ((CAP, 4), u32), ((CAP, 3), f32), ((CAP, 3), i32), (CAP, u8)],
            lambda w, i, o, s: _counts(w.svo1.surface_smooth_device(smooth_params(w), CAP, CAP, *o, s, masks=i[0])), "test_gpu_smooth.py::test_random_caller_masks",
            cpu=smooth_cpu)


def queries(decoy):
    return np.random.default_rng(41 + decoy).integers(-4, RES + 4, (1000, 3)).astype(i32)


def nearest_cpu(which):
    import query_expected as QX
    r = QX.nearest_voxels(SET1[0], SET1[1], queries(which))
    return [r["dist2"], r["nearest"], r["attribs"]]


buffer_case("nearest_voxels", "mvrt_svo_nearest_voxels", lambda: [(queries(0), queries(1))], [(1000, u64), (1000, u32), ((1000, 8), u8)],
            lambda w, i, o, s: w.svo1.nearest_voxels_device(1000, i[0], w.mv.NO_LIMIT, *o, s), "test_gpu_query.py", cpu=nearest_cpu)


# ---- 2. listings with a host count: the input is the handle, rebuilt (or edited) from a device list behind the hold ------------------------------------------------
def listing_case(name, api, outs, call, pinned, cpu=None, edit=False, no_model=""):
    """call( w, svo, outputs, stream ) -> the counts; cpu( xyz, attribs ) -> the model's answer"""
    @case(name, [api, "mvrt_svo_edit_voxels" if edit else "mvrt_svo_build_voxels"], pinned=pinned, no_model=no_model,
          cpu=None if cpu is None else (lambda which: cpu(*(edited(which) if edit else (SET1 if which else SET2)))))
    def make(w):
        r = Run()
        svo = w.mv.IntersectorOctreeGPU()
        r.inputs = handle_inputs(w)
        r.outputs = [w.out(s, d) for s, d in outs]
        if cpu:
            model = cpu(*(edited(0) if edit else SET2))[: len(outs)]
            r.check = lambda got: agrees(got, model)
        r.prepare = lambda: build_from(w, svo, [w.dev(SET1[0]), w.dev(SET1[1])], None)

        def run(stream, which):
            build_from(w, svo, [i[0] for i in r.inputs], stream, edit)
            return call(w, svo, r.outputs, stream)
        r.call = run
        return r


XYZ, ATT, IDX = ((CAP, 3), u32), ((CAP, 8), u8), (CAP, u32)


def sorted_cpu(xyz, at):
    import query_expected as QX
    return [np.asarray(a) for a in QX.sorted_set(xyz, at)]


def walk_cpu(xyz, at):
    v, a = sorted_cpu(xyz, at)
    return [v, np.arange(len(v), dtype=u32), a]


def edited(which):
    """what the edit cases leave: SET1 with the real (SET2) or the decoy (SET1 again) list set over it, the last entry of a voxel winning"""
    if which:
        return SET1
    xyz, at = np.concatenate([SET1[0], SET2[0]]), np.concatenate([SET1[1], SET2[1]])
    _, last = np.unique(morton(xyz[::-1]), return_index=True)
    keep = len(xyz) - 1 - last
    return xyz[keep], at[keep]


def keyed(module, fn, keys, *args, attribs=True):
    def cpu(xyz, at):
        import importlib
        r = getattr(importlib.import_module(module), fn)(*((xyz, at) if attribs else (xyz,)), *args)
        return [np.asarray(r[k]) for k in keys] if keys else [np.asarray(x) for x in (r if isinstance(r, (tuple, list)) else [r])]
    return cpu


listing_case("walk_voxels", "mvrt_svo_walk_voxels", [XYZ, IDX, ATT], lambda w, v, o, s: _counts(v.walk_voxels_device(CAP, *o, s)),
             "test_gpu_walk.py::test_built_handle_walks_like_read_voxels", cpu=walk_cpu)
listing_case("read_voxels", "mvrt_svo_read_voxels", [XYZ, ATT], lambda w, v, o, s: _lib_call(w, "mvrt_svo_read_voxels", v._h, o[0].ptr, o[1].ptr, s),
             "test_gpu_voxel_edit.py::test_read_voxels_round_trip", cpu=sorted_cpu, edit=True)
listing_case("surface_masks", "mvrt_svo_surface_masks", [(CAP, u8)], lambda w, v, o, s: _counts(v.surface_masks_device(o[0], s)), "test_gpu_surface.py",
             cpu=lambda xyz, at: [__import__("surface_expected").masks_of(__import__("surface_expected").sorted_voxels(xyz), RES)])
listing_case("surface_quads", "mvrt_svo_surface_quads", [IDX, (CAP, u8), ((CAP, 4, 3), f32)], lambda w, v, o, s: _counts(v.surface_quads_device(CAP, *o, s)),
             "test_gpu_surface.py", cpu=keyed("surface_expected", "surface", ("faceVoxel", "faceDir", "positions"), RES, VS.LOWER, VS.DPS, attribs=False))
listing_case("surface_mesh", "mvrt_svo_surface_mesh", [IDX, (CAP, u8), ((CAP, 4), u32), ((CAP, 3), f32)],
             lambda w, v, o, s: _counts(v.surface_mesh_device(CAP, CAP, *o, s)), "test_gpu_surface.py",
             cpu=keyed("surface_expected", "surface", ("faceVoxel", "faceDir", "indices", "vertices"), RES, VS.LOWER, VS.DPS, attribs=False))
listing_case("surface_merged", "mvrt_svo_surface_merged", [IDX, (CAP, u8), ((CAP, 2), u32), ((CAP, 4, 3), f32), ((CAP, 4), u32), ((CAP, 3), f32)],
             lambda w, v, o, s: _counts(v.surface_merged_device(2, CAP, CAP, *o, s)), "test_gpu_surface_merge.py", cpu=lambda xyz, at: merged_cpu(xyz, at))
listing_case("surface_exterior_masks", "mvrt_svo_surface_exterior_masks", [(CAP, u8)], lambda w, v, o, s: _counts(v.surface_exterior_masks_device(o[0], s)),
             "test_gpu_exterior.py::test_random_fill", cpu=keyed("exterior_expected", "exterior", ("masks",), RES, attribs=False))
listing_case("enclosed_cells", "mvrt_svo_enclosed_cells", [XYZ, IDX], lambda w, v, o, s: _counts(v.enclosed_cells_device(CAP, *o, s)), "test_gpu_fill.py",
             cpu=keyed("fill_expected", "enclosed", ("xyz", "region"), RES, attribs=False))
listing_case("enclosed_nearest", "mvrt_svo_enclosed_nearest", [XYZ, IDX, IDX, IDX, ATT], lambda w, v, o, s: _counts(v.enclosed_nearest_device(CAP, *o, s)),
             "test_gpu_enclosed_nearest.py::test_agreement_with_the_band_engine", cpu=keyed("nearest_expected", "enclosed_nearest", ("xyz", "region", "dist2", "nearest", "attribs"), RES))
listing_case("coarse_voxels", "mvrt_svo_coarse_voxels", [XYZ, ATT, IDX], lambda w, v, o, s: _counts(v.coarse_voxels_device(1, 2, CAP, *o, s)),
             "test_gpu_coarsen.py::test_random_sets", cpu=keyed("coarsen_expected", "coarse", ("xyz", "attribs", "count"), 1, 2))
listing_case("dilation_cells", "mvrt_svo_dilation_cells", [XYZ, ATT, IDX], lambda w, v, o, s: _counts(v.dilation_cells_device(1, CAP, *o, s)), "test_gpu_morph.py",
             cpu=keyed("morph_expected", "dilation_cells", ("xyz", "attribs", "count"), RES, 1))
listing_case("erosion_voxels", "mvrt_svo_erosion_voxels", [IDX], lambda w, v, o, s: _counts(v.erosion_voxels_device(0, CAP, o[0], s)), "test_gpu_morph.py",
             cpu=keyed("morph_expected", "erosion_voxels", (), RES, 0, attribs=False))
listing_case("distance_cells", "mvrt_svo_distance_cells", [XYZ, IDX, IDX, ATT], lambda w, v, o, s: _counts(v.distance_cells_device(5, CAP, *o, s)), "test_gpu_ball.py",
             cpu=keyed("ball_expected", "distance_cells", ("xyz", "dist2", "nearest", "attribs"), RES, 5))
listing_case("depth_voxels", "mvrt_svo_depth_voxels", [IDX, IDX], lambda w, v, o, s: _counts(v.depth_voxels_device(2, CAP, *o, s)), "test_gpu_ball.py",
             cpu=keyed("ball_expected", "depth_voxels", ("vIndex", "depth2"), RES, 2, attribs=False))
listing_case("components", "mvrt_svo_components", [IDX, IDX, IDX, ((CAP, 6), u32)], lambda w, v, o, s: _counts(v.components_device(1, o[0], CAP, o[1], o[2], o[3], s)),
             "test_gpu_components.py::test_random_sets", cpu=keyed("components_expected", "components", ("label", "size", "first", "box"), RES, 1, attribs=False), edit=True)
listing_case("combine_voxels", "mvrt_svo_combine_voxels", [XYZ, ATT, (CAP, u8)],
             lambda w, v, o, s: _counts(v.combine_voxels_device(w.other, 3, (1, 0, -1), 0, CAP, *o, s)), "test_gpu_combine.py",
             cpu=lambda xyz, at: [np.asarray(x) for x in __import__("combine_expected").combine(xyz, at, SET3[0], SET3[1], RES, 3, (1, 0, -1)).values()][:3])


def merged_cpu(xyz, at):
    import merge_expected as MG
    v, a = sorted_cpu(xyz, at)
    r = MG.merged(v, a, RES, VS.LOWER, VS.DPS, 2)
    return [r[k] for k in ("rectVoxel", "rectDir", "rectSize", "positions", "indices", "vertices")]


SWAP_XY = [[0, 1, 0], [1, 0, 0], [0, 0, 1]]


def resampled_cpu(xyz, at):
    import resample_expected as RX
    r = RX.dense(xyz, at, RES, *RX.from_cells(SWAP_XY), RES)
    return [r["xyz"], r["attribs"], r["source"]]


def between_cpu(xyz, at):
    import query_expected as QX
    r = QX.nearest_between(xyz, SET3[0], (0, 1, 0))
    return [r["dist2"], r["nearest"]]


def swap_xy(w):
    return w.mv.CellTransform.from_cells(SWAP_XY)


listing_case("resample_voxels", "mvrt_svo_resample_voxels", [XYZ, ATT, IDX], lambda w, v, o, s: _counts(v.resample_voxels_device(swap_xy(w), RES, CAP, *o, s)),
             "test_gpu_resample.py", cpu=resampled_cpu)
listing_case("nearest_between", "mvrt_svo_nearest_between", [(CAP, u64), IDX],
             lambda w, v, o, s: [np.array(list(v.nearest_between_device(w.other, (0, 1, 0), w.mv.NO_LIMIT, CAP, o[0], o[1], s).values()), u64)], "test_gpu_query.py",
             cpu=between_cpu)
listing_case("download", "mvrt_svo_download", [], lambda w, v, o, s: list(v.download(True, s)), "test_gpu_voxel_edit.py::test_random_lists_equal_oracle",
             no_model="the expected nodes are the oracle's octree (edit_model.assert_svo: the oracle's build, then a comparison node by node)")


# ---- 3. in-place and handle-producing calls: a trace and a walk follow on the same stream ------------------------------------------------------------------------
def after(w, svo, outs, stream):
    """what follows every in-place call on the stream under test: the rays of the world traced, the voxels listed"""
    w.trace(svo, outs[:3], stream)
    return _counts(svo.walk_voxels_device(CAP, *outs[3:], stream))


def after_outs(w):
    return trace_outs(w) + [w.out(*XYZ), w.out(*IDX), w.out(*ATT)]


def walked(xyz, at):
    """the model's voxel set as the walk half of after() lists it; the trace half stays with the un-held result (ORACLE)"""
    v, a = sorted_cpu(xyz, at) if at is not None else (np.asarray(xyz), None)
    return [None, None, None, v, np.arange(len(v), dtype=u32), a]


def inplace_case(name, apis, op, pinned, edit=False, cpu=sorted_cpu):
    """cpu( xyz, attribs ) -> (xyz, attribs or None) of the set the handle holds after the call, in any order"""
    def model(which):
        return walked(*cpu(*(edited(which) if edit else (SET1 if which else SET2)))[:2])

    @case(name, list(apis) + ["mvrt_svo_edit_voxels" if edit else "mvrt_svo_build_voxels", "mvrt_trace_batch"], pinned=pinned, cpu=model)
    def make(w):
        r = Run()
        svo = w.mv.IntersectorOctreeGPU()
        r.inputs = handle_inputs(w)
        r.outputs = after_outs(w)
        r.check = lambda got: agrees(got, model(0))
        r.prepare = lambda: build_from(w, svo, [w.dev(SET1[0]), w.dev(SET1[1])], None)

        def run(stream, which):
            build_from(w, svo, [i[0] for i in r.inputs], stream, edit)
            more = op(w, svo, stream) if op else None
            return after(w, svo, r.outputs, stream) + _counts(more if more is not None else 0)
        r.call = run
        return r


inplace_case("build_voxels", [], None, "test_gpu_voxel_edit.py::test_random_lists_equal_oracle")
inplace_case("edit_voxels", [], None, "test_gpu_voxel_edit.py::test_edited_octree_traces_like_oracle", edit=True)
inplace_case("rebuild", ["mvrt_svo_rebuild"], lambda w, v, s: v.rebuild(1, s), "test_gpu_walk.py::test_rebuild_of_a_built_handle_changes_the_flavour")
for _op in ("dilate", "erode", "close", "open"):
    inplace_case(_op, ["mvrt_svo_" + _op], lambda w, v, s, _op=_op: getattr(v, _op)(1, 1, s), "test_gpu_morph.py::test_in_place_calls_equal_an_edit_with_the_listing",
                 cpu=lambda xyz, at, _op=_op: __import__("morph_expected").morph(_op, xyz, at, RES, 1, 1))
    inplace_case(_op + "_ball", ["mvrt_svo_%s_ball" % _op], lambda w, v, s, _op=_op: getattr(v, _op + "_ball")(2, s),
                 "test_gpu_ball.py::test_in_place_calls_equal_an_edit_with_the_listing", cpu=lambda xyz, at, _op=_op: __import__("ball_expected").ball(_op, xyz, at, RES, 2))
inplace_case("fill_enclosed", ["mvrt_svo_fill_enclosed"], lambda w, v, s: v.fill_enclosed(np.arange(8, dtype=u8), s), "test_gpu_fill.py",
             cpu=lambda xyz, at: (__import__("fill_expected").filled_set(xyz, RES), None))  # (the model gives the set; the fill colour is the un-held result's)
inplace_case("fill_enclosed_nearest", ["mvrt_svo_fill_enclosed_nearest"], lambda w, v, s: v.fill_enclosed_nearest(s),
             "test_gpu_enclosed_nearest.py::test_fill_equals_an_edit_with_the_models_cells", cpu=lambda xyz, at: __import__("nearest_expected").filled(xyz, at, RES))
inplace_case("keep_components", ["mvrt_svo_keep_components"], lambda w, v, s: v.keep_components(1, 5, 0, s), "test_gpu_components.py::test_min_voxels_around_a_size",
             cpu=lambda xyz, at: __import__("components_expected").keep(xyz, at, RES, 1, 5, 0))
inplace_case("combine", ["mvrt_svo_combine"], lambda w, v, s: v.combine(w.other, 0, (1, 0, -1), 1, s), "test_gpu_combine.py",
             cpu=lambda xyz, at: list(__import__("combine_expected").combine(xyz, at, SET3[0], SET3[1], RES, 0, (1, 0, -1), 1).values()))
inplace_case("resample", ["mvrt_svo_resample"], lambda w, v, s: v.resample(swap_xy(w), stream=s) and None, "test_gpu_resample.py", cpu=resampled_cpu)
inplace_case("coarsen", ["mvrt_svo_coarsen"], lambda w, v, s: v.coarsen(1, 1, stream=s) and None, "test_gpu_coarsen.py::test_in_place_and_over_another_octree",
             cpu=keyed("coarsen_expected", "coarse", ("xyz", "attribs"), 1, 1))
inplace_case("transfer_attributes", ["mvrt_svo_transfer_attributes"], lambda w, v, s: v.transfer_attributes(w.other, None, 9, 3, s), "test_gpu_query.py",
             cpu=lambda xyz, at: __import__("query_expected").transferred(xyz, at, SET3[0], SET3[1], (0, 0, 0), 9, 3))
inplace_case("set_emission_scale", [], lambda w, v, s: v.set_emission_scale(3.0), "test_gpu_parity.py::test_trace_batch_bit_exact")


@case("lod_prepare", ["mvrt_svo_lod_prepare", "mvrt_svo_build_voxels", "mvrt_trace_batch_cone"], pinned="test_gpu_cone.py::test_pyramid_goes_with_the_voxels_it_describes",
      no_model="the expected cone hits are lod_expected's tree walk: a tree from the oracle scene (lod_expected.scene), then its trace")
def _lod_prepare(w):
    r = Run()
    svo = w.mv.IntersectorOctreeGPU()
    r.inputs = handle_inputs(w)
    r.outputs = [w.out(N_RAYS, f32), w.out(N_RAYS, i32), w.out(N_RAYS, u32), w.out(N_RAYS, u64), w.out(N_RAYS, u32), w.out((N_RAYS, 8), u8), w.out(N_RAYS, u32)]
    r.prepare = lambda: build_from(w, svo, [w.dev(SET1[0]), w.dev(SET1[1])], None)
    cones = [w.dev(RAYS[8]), w.dev(RAYS[9])]

    def run(stream, which):
        build_from(w, svo, [i[0] for i in r.inputs], stream)
        svo.lod_prepare(stream)
        svo.intersect_cone_device(N_RAYS, *w.rays[:6], *cones, *r.outputs, stream)
    r.call = run
    return r


def host_build_case(name, apis, build, pinned, cpu=None, no_model=""):
    """host inputs only (no regime C): build( w, svo, which, stream ) from the real (0) or the decoy (1) host data"""
    @case(name, list(apis) + ["mvrt_trace_batch", "mvrt_svo_walk_voxels"], device_inputs=False, pinned=pinned, cpu=cpu, no_model=no_model)
    def make(w):
        r = Run()
        svo = w.mv.IntersectorOctreeGPU()
        r.outputs = after_outs(w)
        if cpu:
            r.check = lambda got: agrees(got, cpu(0))
        r.prepare = lambda: build(w, svo, 1, None)

        def run(stream, which):
            build(w, svo, which, stream)
            return after(w, svo, r.outputs, stream)
        r.call = run
        return r


def _upload(w, svo, which, stream):
    if not hasattr(w, "uploads"):
        w.uploads = []
        for xyz, at in (SET2, SET1):
            nodes, attrs, _ = VS.build(w.mv, xyz, RES, attribs=at).download()
            w.uploads.append((nodes, attrs, int(attrs[:, 4:7].any())))
    nodes, attrs, he = w.uploads[which]
    svo.upload(nodes, attrs, VS.LOWER, VS.DPS, RES, he, True, stream)


VOXELISED = "the expected voxels are the oracle's voxelisation of the triangles (O.build_scene_from_triangles on this lattice, then its voxel list)"
host_build_case("build", ["mvrt_svo_build"], lambda w, v, k, s: _lib_call(
    w, "mvrt_svo_build", v._h, w.tris[k][0].ctypes.data_as(C.c_void_p), w.tris[k][1].ctypes.data_as(C.c_void_p), w.tris[k][2].ctypes.data_as(C.c_void_p), len(w.tris[k][0]), s,
    VS.LOWER.ctypes.data_as(C.c_void_p), float(VS.DPS), RES), "test_gpu_build.py::test_bunny_with_attributes_and_emission", no_model=VOXELISED)
host_build_case("build_ex", ["mvrt_svo_build_ex"], lambda w, v, k, s: v.build(*w.tris[k], s, VS.LOWER, VS.DPS, RES, 1 | 4), "test_gpu_build.py::test_conservative_voxelization_mode",
                no_model=VOXELISED)
host_build_case("build_synthetic", ["mvrt_svo_build_synthetic"], lambda w, v, k, s: v.build_synthetic(RES, N_VOXELS, 7 + k, VS.LOWER, VS.DPS, 0, s), "test_gpu_build.py",
                no_model="rays.synthetic_reference restates the generator and then needs the oracle's Morton codes and merge")
host_build_case("upload", ["mvrt_svo_upload"], _upload, "test_gpu_walk.py::test_walk_of_every_legal_shape", cpu=lambda which: walked(*(SET1 if which else SET2)))


# ---- 4. the path tracer -----------------------------------------------------------------------------------------------------------------------------------------
SETUP_APIS = ["mvrt_pt_setup", "mvrt_pt_load_hdri", "mvrt_pt_update_scene", "mvrt_pt_resize_framebuffer_if_needed", "mvrt_pt_clear_framebuffer"]


def pt_case(name, apis, body, options=(), device_inputs=False, setup_inside=False, pinned="test_gpu_parity.py::test_path_tracer_bit_exact", check=None):
    """body( w, pt, stream, which, run ) -> host results; `which` picks the camera (a host input).  The path tracer is made for every regime: setup, the switches
    named in `options`, load_hdri, update_scene, resize, clear.  That happens on the default stream BEFORE the window opens, since setup, load_hdri and
    update_scene each end in a wait for their stream and free scratch, which would use the hold up before the body's first call; the body then runs with the
    hold still in force.  setup_inside: the one case that makes those five calls on the stream under test, behind the hold"""
    @case(name, (SETUP_APIS if setup_inside else []) + list(apis), device_inputs=device_inputs, pinned=pinned, no_model=FRAME)
    def make(w):
        r = Run()
        n_owned = 256  # 17 x 13 = 221 pixels, padded to a tile
        if device_inputs:
            r.inputs = [(w.dev(sample_mask(True, n_owned)), sample_mask(False, n_owned), sample_mask(True, n_owned))]
        r.scratch = [w.out((n_owned, 4), f32) for _ in range(2)] + [w.out((n_owned, 4), u8), w.out(n_owned, u8)]

        def fresh(stream):
            pt = w.mv.PathTracer()
            w.keep.append(pt)
            pt.setup(stream)
            for k in options:
                getattr(pt, k)(True)
            pt.loadHDRIPixels(stream, w.rgba, w.hw, w.hh, w.rgba, w.hw, w.hh)
            v, c, e = w.tris[0]
            _lib_call(w, "mvrt_pt_update_scene", pt._h, v.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p), len(v), stream,
                      VS.LOWER.ctypes.data_as(C.c_void_p), float(VS.DPS), RES)
            pt.resizeFrameBufferIfNeeded(stream, W, H)
            pt.clearFrameBuffer(stream)
            assert pt.owned_pixels() == n_owned
            return pt

        r.fresh = fresh
        if not setup_inside:
            def prepare():
                r.pt = fresh(None)
            r.prepare = prepare
        r.call = lambda stream, which: body(w, fresh(stream) if setup_inside else r.pt, stream, which, r)
        if check:
            r.check = lambda got: check(w, r, got)
        return r


def steps(pt, stream, which, n=STEPS):
    for _ in range(n):
        pt.step(stream, camera(which))


def dev_read(w, ptr, like, stream):
    """a device read of one of the handle's buffers on the stream under test, waiting for that stream only"""
    w.mv.memcpy_d2d(like, ptr, like.nbytes, stream)
    w.st.sync(stream)
    return like.to_host()


def _pt_join(w, pt, stream, which, r):
    steps(pt, stream, which)
    pt.join(stream)
    return [dev_read(w, pt.framebuffer_dev(), r.scratch[0], stream)]


def _pt_read(w, pt, stream, which, r):
    steps(pt, stream, which)
    return [pt.read_framebuffer(stream)]


def _pt_stats(w, pt, stream, which, r):
    steps(pt, stream, which)
    return [tallies(pt, stream)]


def _pt_resolve(w, pt, stream, which, r):
    steps(pt, stream, which)
    pt.resolve(stream)
    return [dev_read(w, w.mv.lib().mvrt_pt_framebuffer_u8_dev(pt._h), r.scratch[2], stream)[: W * H]]  # (the padding of the last tile is never written)


def _pt_to_image(w, pt, stream, which, r):
    steps(pt, stream, which)
    image = pt.toImageAsync(stream)
    w.st.sync(stream)
    return [image[: W * H].copy()]


def _pt_setup(w, pt, stream, which, r):
    """the five set-up calls were made behind the hold (setup_inside); the map is loaded once more from its file, then a frame"""
    pt.loadHDRI(stream, os.path.join(GOLDEN, "monks_forest_s.hdr"))
    steps(pt, stream, which)
    return [pt.read_framebuffer(stream)]


def _pt_matrices(w, pt, stream, which, r):
    for _ in range(STEPS):
        pt.step(stream, look_at(which), 0.5, 0.002)
    return [pt.read_framebuffer(stream)]


def tallies(pt, stream):
    return np.array(list(pt.stats(stream).values())[:6], np.float64)


def _pt_reset_stats(w, pt, stream, which, r):
    """mvrt_pt_reset_stats clears the tallies on the default stream; the step after it tallies on a slot stream that does not wait for the default stream"""
    steps(pt, stream, 1 - which, 1)
    pt.reset_stats()
    steps(pt, stream, which, 1)
    return [tallies(pt, stream)]


def _second_step_only(w, r, got):
    """the tallies after the reset are those of the second step alone: the difference of two un-reset readings"""
    pt = r.fresh(None)
    steps(pt, None, 1, 1)
    first = tallies(pt, None)
    steps(pt, None, 0, 1)
    return np.array_equal(got[0], tallies(pt, None) - first) and got[0][1] > 0


def _pt_clear_between(w, pt, stream, which, r):
    steps(pt, stream, 1 - which, 1)  # a first frame from the other camera: the second frame must not contain it
    pt.clearFrameBuffer(stream)
    steps(pt, stream, which, 1)
    pt.join(stream)
    return [dev_read(w, pt.framebuffer_dev(), r.scratch[0], stream)]


def after_steps(call):
    """a body: the steps, then ONE call that reads back, so that it is the first to wait behind the hold"""
    def body(w, pt, stream, which, r):
        steps(pt, stream, which)
        return call(w, pt, stream, r)
    return body


def _denoised_dev(w, pt, stream, r):
    pt.denoise(stream, iterations=2)
    return [dev_read(w, pt.denoised_dev(), w.tmp((W * H, 4), f32), stream)]


def _read_denoised(w, pt, stream, r):
    pt.denoise(stream, iterations=2)
    return [pt.read_denoised(stream)]


def _error_mask(w, pt, stream, r):
    _, n = pt.error_mask(0.05, min_samples=16, out_dev=r.scratch[3], stream=stream)
    return [dev_read(w, r.scratch[3].ptr, w.tmp(256, u8), stream), np.array([n])]


def _pt_mask(w, pt, stream, which, r):
    steps(pt, stream, 0, 1)
    n = pt.set_sample_mask(r.inputs[0][0], stream)
    steps(pt, stream, 0, 1)
    return [pt.read_framebuffer(stream), np.array([n])]


pt_case("pt_setup_to_first_frame", ["mvrt_pt_load_hdri_file", "mvrt_pt_step", "mvrt_pt_read_framebuffer"], _pt_setup, setup_inside=True)
pt_case("pt_join_framebuffer_dev", ["mvrt_pt_step", "mvrt_pt_join"], _pt_join)
pt_case("pt_read_framebuffer", ["mvrt_pt_step", "mvrt_pt_read_framebuffer"], _pt_read)
pt_case("pt_get_stats", ["mvrt_pt_step", "mvrt_pt_get_stats"], _pt_stats, pinned="test_gpu_parity.py::test_path_tracer_bit_exact (ray statistics)")
pt_case("pt_resolve", ["mvrt_pt_step", "mvrt_pt_resolve"], _pt_resolve)
pt_case("pt_to_image_async", ["mvrt_pt_step", "mvrt_pt_to_image_async"], _pt_to_image)
pt_case("pt_step_matrices", ["mvrt_pt_step_matrices", "mvrt_pt_read_framebuffer"], _pt_matrices,
        pinned="test_gpu_parity.py::test_path_tracer_bit_exact (matrices: test_gpu_build.py::test_update_scene_then_step_matches_oracle)")
pt_case("pt_clear_between_steps", ["mvrt_pt_step", "mvrt_pt_clear_framebuffer", "mvrt_pt_join"], _pt_clear_between)
pt_case("pt_read_aov_albedo", ["mvrt_pt_step", "mvrt_pt_read_aov"], after_steps(lambda w, pt, s, r: [pt.read_aov(0, s)]), options=("set_aovs", "set_moments"),
        pinned="test_gpu_aov.py::test_feature_buffers_bit_exact")
pt_case("pt_read_aov_normal_depth", ["mvrt_pt_step", "mvrt_pt_read_aov"], after_steps(lambda w, pt, s, r: [pt.read_aov(1, s)]), options=("set_aovs", "set_moments"),
        pinned="test_gpu_aov.py::test_feature_buffers_bit_exact")
pt_case("pt_read_moments", ["mvrt_pt_step", "mvrt_pt_read_moments"], after_steps(lambda w, pt, s, r: [pt.read_moments(s)]), options=("set_aovs", "set_moments"),
        pinned="test_gpu_denoise.py::test_moments_bit_exact_and_nothing_else_moves")
pt_case("pt_denoise_denoised_dev", ["mvrt_pt_step", "mvrt_pt_denoise"], after_steps(_denoised_dev), options=("set_aovs", "set_moments"), pinned="test_gpu_denoise.py::test_denoiser_equals_the_contract")
pt_case("pt_denoise_read_denoised", ["mvrt_pt_step", "mvrt_pt_denoise", "mvrt_pt_read_denoised"], after_steps(_read_denoised), options=("set_aovs", "set_moments"),
        pinned="test_gpu_denoise.py::test_denoiser_equals_the_contract")
pt_case("pt_error_mask", ["mvrt_pt_step", "mvrt_pt_error_mask"], after_steps(_error_mask), options=("set_aovs", "set_moments"), pinned="test_gpu_adaptive.py (error mask)")
pt_case("pt_set_sample_mask", ["mvrt_pt_step", "mvrt_pt_set_sample_mask", "mvrt_pt_read_framebuffer"], _pt_mask, device_inputs=True, pinned="test_gpu_adaptive.py")
pt_case("pt_reset_stats_between_steps", ["mvrt_pt_step", "mvrt_pt_get_stats"], _pt_reset_stats, check=_second_step_only,
        pinned="test_gpu_parity.py::test_path_tracer_bit_exact (ray statistics)")

EXEMPT = ("mvrt_stream_create", "mvrt_stream_destroy", "mvrt_stream_synchronize", "mvrt_memcpy_h2d", "mvrt_memcpy_d2h", "mvrt_memcpy_d2d")  # the harness's own tools


# ---- the regimes ------------------------------------------------------------------------------------------------------------------------------------------------
def regime(w, r, mode):
    """mode: 'real' / 'decoy' = the default stream, nothing held; 'A', 'B', 'C' as in the module's docstring -> the host results"""
    st, mv = w.st, w.mv
    S = st.S
    r.prepare()
    first = 0 if mode == "real" else 1
    for dev, real, decoy in r.inputs:
        rc = mv.lib().mvrt_memcpy_h2d(dev.ptr, np.ascontiguousarray((real, decoy)[first]).ctypes.data_as(C.c_void_p), dev.nbytes, None)
        assert rc == 0
    for o in r.outputs:
        zero = np.zeros(o.nbytes, u8)
        assert mv.lib().mvrt_memcpy_h2d(o.ptr, zero.ctypes.data_as(C.c_void_p), o.nbytes, None) == 0
    sources = [w.dev(real) for _, real, _ in r.inputs]  # the producer's data, resident before the window opens
    mv.synchronize()
    if mode in ("real", "decoy"):
        t0 = time.perf_counter()
        more = r.call(None, first)
        CALL_MS[mode].append((time.perf_counter() - t0) * 1e3)
        got, copies = st.snapshot(r.outputs, None)
    else:
        fill_on, call_on, held = {"A": (S, S, S), "B": (S, S, None), "C": (S, None, S)}[mode]
        with st.held(held):
            for (dev, _, _), src in zip(r.inputs, sources):
                st.async_fill(dev, src, fill_on)
            more = r.call(call_on, 0)
            got, copies = st.snapshot(r.outputs, call_on)
    mv.synchronize()
    del copies, sources
    return got + list(more or [])


@pytest.fixture(scope="module")
def world(streams):  # noqa: F811
    w = World(streams)
    yield w
    w.mv.synchronize()
    w.keep.clear()
    if CALL_MS["decoy"]:
        print("un-held calls on the default stream: longest %.2f ms first, %.2f ms second; all second: %s" % (
            max(CALL_MS["real"]), max(CALL_MS["decoy"]), " ".join("%.2f" % t for t in CALL_MS["decoy"])))


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_stream_order(world, c):
    w = world
    tag = "stream-order[%s]" % c.name
    try:
        check_case(w, c, tag)
    except w.mv.MvrtError as e:
        if " failed: " not in str(e) or "hip" not in str(e):  # a call the library refused (REQUIRE): the device is healthy, the case fails
            raise
        # a HIP call failed (the text of MVRT_HIP): this ends the whole pytest session, so that nothing more is started on a device in error
        pytest.exit("%s: %s" % (tag, e), returncode=3)
    finally:
        w.keep.clear()


def check_case(w, c, tag):
    r = c.make(w)
    want, decoy = regime(w, r, "real"), regime(w, r, "decoy")
    assert not same(want, decoy), "%s: the real and the decoy inputs give the same result on the default stream: the case cannot see a mis-ordering" % tag
    if r.check:
        assert r.check(want), "%s: the un-held result differs from the CPU model" % tag
    for mode in ("A", "B"):
        got = regime(w, r, mode)
        print("%s regime %s: %d of %d values differ" % (tag, mode, differing(got, want), total(want)))
        assert same(got, want), "%s regime %s: %d of %d values differ%s" % (tag, mode, differing(got, want), total(want),
                                                                             " (the result is the decoy's)" if same(got, decoy) else "")
    if c.device_inputs:
        got = regime(w, r, "C")
        print("%s regime C: the planted mis-ordering gave %s" % (tag, "the decoy's result" if same(got, decoy) else "the real result" if same(got, want) else "a third result"))
        assert not same(got, want), "%s regime C: hold did not outlast the call: made on the default stream, it still saw the input queued behind the hold" % tag


def test_a_trace_queued_before_an_in_place_edit_sees_the_old_octree(world):
    """the other way round: a trace waits behind the hold on S, then the handle is dilated on S: the trace's result is the old octree's, and nothing faults, since
    the old arrays outlive the queued kernel (the edit drains the stream before it releases them)"""
    w = world
    svo = VS.build(w.mv, SET1[0], RES, attribs=SET1[1])
    outs = trace_outs(w)
    w.trace(svo, outs, None)
    old, keep = w.st.snapshot(outs, None)
    with w.st.held(w.st.S):
        w.trace(svo, outs, w.st.S)
        added = svo.dilate(1, 1, w.st.S)
        got, keep2 = w.st.snapshot(outs, w.st.S)
    w.mv.synchronize()
    assert added > 0 and same(got, old), "stream-order[trace before dilate]: %d of %d values differ" % (differing(got, old), total(old))
    w.trace(svo, outs, w.st.S)
    new, keep3 = w.st.snapshot(outs, w.st.S)
    assert not same(new, old)
