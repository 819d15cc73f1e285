"""massivevoxelraytracing_amd -- MI355X-native SVO path tracer behind the reference's host API.

Python mirror of the reference's two host structs for the GPU hot path:

* ``IntersectorOctreeGPU``  (reference IntersectorOctreeGPU.hpp:21-275)
* ``PathTracer``            (reference PathTracer.hpp:14-170)

Both are thin ctypes views over the C-ABI library ``libmvrt_hip.so`` (include/mvrt.h) -- the same
entry points a C++ caller binds through include/mvrt/*.hpp.  There is NO CPU fallback: importing
``lib()`` fails loudly if the HIP library is missing or cannot be loaded.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MVRT_LIB", os.path.join(_HERE, "libmvrt_hip.so"))  # MVRT_LIB: A/B builds of the same library
MAX_FLOAT = np.float32(3.402823466e38)

_vp, _i32, _u32, _u64, _f32 = C.c_void_p, C.c_int, C.c_uint32, C.c_uint64, C.c_float


class MvrtError(RuntimeError):
    pass


class SvoInfo(C.Structure):
    _fields_ = [("numberOfNodes", _u32), ("numberOfVoxels", _u32), ("lower", _f32 * 3), ("upper", _f32 * 3), ("dps", _f32), ("emissionScale", _f32),
                ("hasEmission", _u32), ("embeddedMask", _u32), ("gridRes", _u32), ("levels", _u32), ("totalDumpedVoxels", _u64), ("flavour", _u32), ("reserved", _u32)]


class DeviceOctree(C.Structure):
    """mvrt_device_octree (include/mvrt.h): the device view a user kernel takes by value (include/mvrt/device.hpp)"""
    _fields_ = [("structBytes", _u32), ("flavour", _u32), ("nodes", _u64), ("kids", _u64), ("masks", _u64), ("psumCold", _u64), ("attrs", _u64),
                ("cellBlocks", _u64), ("cellEntries", _u64), ("lower", _f32 * 3), ("upper", _f32 * 3), ("dps", _f32), ("emissionScale", _f32),
                ("hasEmission", _u32), ("levels", _u32), ("numberOfNodes", _u32), ("numberOfVoxels", _u32), ("rootIndex", _u32), ("rootMask", _u32),
                ("treeRoot", _u32), ("cellBits", _u32)]


class DeviceLod(C.Structure):
    """mvrt_device_lod (include/mvrt.h): the view of the attribute pyramid a user kernel takes by value (mvrt::DeviceLod, include/mvrt/device.hpp)"""
    _fields_ = [("structBytes", _u32), ("levels", _u32), ("codes", _u64 * 17), ("attrs", _u64 * 17), ("cellVoxels", _u64 * 17), ("count", _u32 * 17), ("reserved", _u32)]


class PtStats(C.Structure):
    _fields_ = [("samples", _u64), ("rays", _u64), ("shadowRays", _u64), ("descents", _u64), ("shadowDescents", _u64), ("hits", _u64), ("traceLaunches", _u64),
                ("traceKernelMs", C.c_double), ("shadeKernelMs", C.c_double), ("totalKernelMs", C.c_double)]


class DenoiseParams(C.Structure):
    """mvrt_denoise_params (include/mvrt.h)"""
    _fields_ = [("structBytes", _u32), ("iterations", C.c_int32), ("sigmaNormal", _f32), ("sigmaDepth", _f32), ("sigmaCoverage", _f32), ("sigmaLuminance", _f32),
                ("albedoFloor", _f32), ("flags", _u32), ("reserved", _u32 * 2)]


class SmoothParams(C.Structure):
    """mvrt_smooth_params (include/mvrt.h)"""
    _fields_ = [("iterations", C.c_int32), ("weightEven", C.c_int32), ("weightOdd", C.c_int32), ("limit", C.c_int32), ("reserved", _u32 * 4)]


class CellTransform(C.Structure):
    """mvrt_cell_transform (include/mvrt.h): the inverse map, destination cell space to source cell space, m row-major in Q24 and t in Q25.
    CellTransform.make(m, t) takes 9 and 3 Python ints as they are; from_cells(A, b) rounds a real 3x3 matrix and translation in cell units."""
    _fields_ = [("structBytes", _u32), ("reserved", _u32), ("m", C.c_int64 * 9), ("t", C.c_int64 * 3)]

    @classmethod
    def make(cls, m, t):
        x = cls()
        x.structBytes, x.reserved = C.sizeof(cls), 0
        x.m[:] = [int(v) for v in np.asarray(m, object).reshape(9)]
        x.t[:] = [int(v) for v in np.asarray(t, object).reshape(3)]
        return x

    @classmethod
    def from_cells(cls, A, b=(0.0, 0.0, 0.0)):
        """s = A c + b in cell coordinates (c the destination point, s the source point): m = rint(A * 2^24), t = rint(b * 2^25)"""
        A, b = np.asarray(A, np.float64).reshape(9), np.asarray(b, np.float64).reshape(3)
        return cls.make([int(v) for v in np.rint(A * 2.0 ** TRANSFORM_FRAC_BITS)], [int(v) for v in np.rint(b * 2.0 ** (TRANSFORM_FRAC_BITS + 1))])

    def arrays(self):
        """(m (9,) int64, t (3,) int64)"""
        return np.array(self.m[:], np.int64), np.array(self.t[:], np.int64)


TRANSFORM_FRAC_BITS = 24  # MVRT_TRANSFORM_FRAC_BITS
DENOISE_NO_DEMODULATION = 1
SURFACE_MERGE_ANY_ATTRIBUTE = 1  # mvrt_svo_surface_merged flags (include/mvrt.h)
SURFACE_MERGE_WELD = 2
MORPH_FACES = 0  # structuring elements of dilate / erode / close / open (include/mvrt.h)
MORPH_CUBE = 1
COMBINE_UNION, COMBINE_INTERSECTION, COMBINE_DIFFERENCE, COMBINE_XOR = 0, 1, 2, 3  # mvrt_svo_combine_voxels / mvrt_svo_combine ops (include/mvrt.h)
COMBINE_ATTRIB_B = 1  # flags: the surviving overlap takes b's attributes
TRANSFER_COLOUR, TRANSFER_EMISSION = 1, 2  # mvrt_svo_transfer_attributes flags (include/mvrt.h)
NO_LIMIT = (1 << 64) - 1  # maxDist2 of the nearest-voxel calls: UINT64_MAX = no limit; also the dist2 of a query beyond the limit


# every symbol include/mvrt.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "mvrt_last_error": (C.c_char_p, []),
    "mvrt_device_count": (_i32, [_vp]),
    "mvrt_set_device": (_i32, [_i32]),
    "mvrt_device_name": (_i32, [_vp, _i32]),
    "mvrt_stream_create": (_i32, [_vp]),
    "mvrt_stream_destroy": (_i32, [_vp]),
    "mvrt_stream_synchronize": (_i32, [_vp]),
    "mvrt_device_synchronize": (_i32, []),
    "mvrt_malloc": (_i32, [_vp, _u64]),
    "mvrt_free": (_i32, [_vp]),
    "mvrt_memcpy_h2d": (_i32, [_vp, _vp, _u64, _vp]),
    "mvrt_memcpy_d2h": (_i32, [_vp, _vp, _u64, _vp]),
    "mvrt_memcpy_d2d": (_i32, [_vp, _vp, _u64, _vp]),
    "mvrt_svo_create": (_i32, [_vp]),
    "mvrt_svo_destroy": (_i32, [_vp]),
    "mvrt_svo_build": (_i32, [_vp, _vp, _vp, _vp, _u64, _vp, _vp, _f32, _i32]),
    "mvrt_svo_build_ex": (_i32, [_vp, _vp, _vp, _vp, _u64, _vp, _vp, _f32, _i32, _i32]),
    "mvrt_svo_build_synthetic": (_i32, [_vp, _i32, _u64, _u64, _vp, _f32, _i32, _vp]),
    "mvrt_svo_upload": (_i32, [_vp, _vp, _u32, _vp, _u32, _vp, _f32, _i32, _i32, _i32, _vp]),
    "mvrt_svo_check_upload": (_i32, [_vp, _u32, _u32, _i32, _i32]),
    "mvrt_svo_build_voxels": (_i32, [_vp, _vp, _vp, _u64, _vp, _f32, _i32, _i32, _vp]),
    "mvrt_svo_edit_voxels": (_i32, [_vp, _vp, _vp, _vp, _u64, _vp]),
    "mvrt_svo_read_voxels": (_i32, [_vp, _vp, _vp, _vp]),
    "mvrt_svo_walk_voxels": (_i32, [_vp, _u64, _vp, _vp, _vp, _vp, _vp]),
    "mvrt_svo_rebuild": (_i32, [_vp, _i32, _vp]),
    "mvrt_svo_surface_masks": (_i32, [_vp, _vp, _vp, _vp]),
    "mvrt_svo_surface_quads": (_i32, [_vp, _u64, _vp, _vp, _vp, _vp, _vp]),
    "mvrt_svo_surface_mesh": (_i32, [_vp, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mvrt_svo_surface_merged": (_i32, [_vp, _u32, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mvrt_svo_surface_exterior_masks": (_i32, [_vp, _vp, _vp, _vp, _vp]),
    "mvrt_svo_surface_quads_masked": (_i32, [_vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp]),
    "mvrt_svo_surface_mesh_masked": (_i32, [_vp, _vp, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mvrt_svo_surface_merged_masked": (_i32, [_vp, _vp, _u32, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mvrt_smooth_default_params": (_i32, [_vp]),
    "mvrt_svo_surface_smooth": (_i32, [_vp, _vp, _vp, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mvrt_svo_enclosed_cells": (_i32, [_vp, _u64, _vp, _vp, _vp, _vp, _vp]),
    "mvrt_svo_fill_enclosed": (_i32, [_vp, _vp, _vp, _vp]),
    "mvrt_svo_enclosed_nearest": (_i32, [_vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mvrt_svo_fill_enclosed_nearest": (_i32, [_vp, _vp, _vp]),
    "mvrt_svo_coarse_voxels": (_i32, [_vp, _i32, _u64, _u64, _vp, _vp, _vp, _vp, _vp]),
    "mvrt_svo_coarsen": (_i32, [_vp, _vp, _i32, _u64, _i32, _vp]),
    "mvrt_svo_dilation_cells": (_i32, [_vp, _i32, _u64, _vp, _vp, _vp, _vp, _vp]),
    "mvrt_svo_erosion_voxels": (_i32, [_vp, _i32, _u64, _vp, _vp, _vp]),
    "mvrt_svo_components": (_i32, [_vp, _i32, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mvrt_svo_keep_components": (_i32, [_vp, _i32, _u64, C.c_uint32, _vp, _vp, _vp]),
    "mvrt_svo_combine_voxels": (_i32, [_vp, _vp, _i32, _vp, _u32, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mvrt_svo_combine": (_i32, [_vp, _vp, _i32, _vp, _u32, _vp, _vp, _vp, _vp]),
    "mvrt_svo_resample_voxels": (_i32, [_vp, _vp, _i32, _u64, _vp, _vp, _vp, _vp, _vp]),
    "mvrt_svo_resample": (_i32, [_vp, _vp, _vp, _vp, _f32, _i32, _i32, _vp, _vp]),
    "mvrt_cell_transform_from_world": (_i32, [_vp, _vp, _f32, _vp, _f32, _vp]),
    "mvrt_svo_nearest_voxels": (_i32, [_vp, _u64, _vp, _u64, _vp, _vp, _vp, _vp]),
    "mvrt_svo_nearest_between": (_i32, [_vp, _vp, _vp, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mvrt_svo_transfer_attributes": (_i32, [_vp, _vp, _vp, _u64, _u32, _vp, _vp, _vp]),
    "mvrt_svo_dilate": (_i32, [_vp, _i32, _i32, _vp, _vp]),
    "mvrt_svo_erode": (_i32, [_vp, _i32, _i32, _vp, _vp]),
    "mvrt_svo_close": (_i32, [_vp, _i32, _i32, _vp, _vp]),
    "mvrt_svo_open": (_i32, [_vp, _i32, _i32, _vp, _vp]),
    "mvrt_svo_distance_cells": (_i32, [_vp, _u32, _u64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mvrt_svo_depth_voxels": (_i32, [_vp, _u32, _u64, _vp, _vp, _vp, _vp]),
    "mvrt_svo_dilate_ball": (_i32, [_vp, _u32, _vp, _vp]),
    "mvrt_svo_erode_ball": (_i32, [_vp, _u32, _vp, _vp]),
    "mvrt_svo_close_ball": (_i32, [_vp, _u32, _vp, _vp]),
    "mvrt_svo_open_ball": (_i32, [_vp, _u32, _vp, _vp]),
    "mvrt_svo_get_info": (_i32, [_vp, _vp]),
    "mvrt_svo_set_emission_scale": (_i32, [_vp, _f32]),
    "mvrt_svo_device_view": (_i32, [_vp, _vp]),
    "mvrt_svo_traversal_bytes": (_u64, [_vp]),
    "mvrt_svo_node_buffer_dev": (_vp, [_vp]),
    "mvrt_svo_attribute_buffer_dev": (_vp, [_vp]),
    "mvrt_pt_download_pmj": (_i32, [_vp, _vp]),
    "mvrt_svo_download": (_i32, [_vp, _vp, _vp, _vp, _vp]),
    "mvrt_trace_batch": (_i32, [_vp, _u64] + [_vp] * 11 + [_vp]),
    "mvrt_trace_batch_hinted": (_i32, [_vp, _u64] + [_vp] * 12 + [_vp]),
    "mvrt_trace_batch_host": (_i32, [_vp, _u64] + [_vp] * 7),
    "mvrt_trace_batch_range": (_i32, [_vp, _u64] + [_vp] * 12 + [_vp]),
    "mvrt_trace_batch_cone": (_i32, [_vp, _u64] + [_vp] * 15 + [_vp]),
    "mvrt_render_primary_lod": (_i32, [_vp, _vp, _i32, _i32, _f32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mvrt_svo_lod_prepare": (_i32, [_vp, _vp]),
    "mvrt_svo_lod_release": (_i32, [_vp]),
    "mvrt_svo_lod_bytes": (_u64, [_vp]),
    "mvrt_svo_lod_view": (_i32, [_vp, _vp]),
    "mvrt_ao_directions": (_i32, [_i32, _vp]),
    "mvrt_svo_surface_ao": (_i32, [_vp, _u64, _vp, _vp, _i32, _f32, _vp, _vp]),
    "mvrt_render_primary": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mvrt_camera_from_matrices": (_i32, [_vp, _vp, _f32, _f32, _vp]),
    "mvrt_compact_indices": (_i32, [_vp, _u64, _vp, _vp, _vp]),
    "mvrt_pt_create": (_i32, [_vp]),
    "mvrt_pt_destroy": (_i32, [_vp]),
    "mvrt_pt_setup": (_i32, [_vp, _vp]),
    "mvrt_pt_resize_framebuffer_if_needed": (_i32, [_vp, _vp, _i32, _i32]),
    "mvrt_pt_clear_framebuffer": (_i32, [_vp, _vp]),
    "mvrt_pt_load_hdri": (_i32, [_vp, _vp, _vp, _i32, _i32, _vp, _i32, _i32]),
    "mvrt_pt_load_hdri_file": (_i32, [_vp, _vp, C.c_char_p, C.c_char_p]),
    "mvrt_pt_download_hdri_sat": (_i32, [_vp, _i32, _vp]),
    "mvrt_rgbe_read_file": (_i32, [C.c_char_p, _vp, _u64, _vp, _vp]),
    "mvrt_pt_set_hdri_scale": (_i32, [_vp, _f32]),
    "mvrt_pt_update_scene": (_i32, [_vp, _vp, _vp, _vp, _u64, _vp, _vp, _f32, _i32]),
    "mvrt_pt_intersector": (_vp, [_vp]),
    "mvrt_pt_step": (_i32, [_vp, _vp, _vp]),
    "mvrt_pt_step_matrices": (_i32, [_vp, _vp, _vp, _vp, _f32, _f32]),
    "mvrt_pt_set_pipeline_depth": (_i32, [_vp, _i32]),
    "mvrt_pt_set_origin_hints": (_i32, [_vp, _i32]),
    "mvrt_pt_set_batch_steps": (_i32, [_vp, _i32]),
    "mvrt_pt_set_split_small_passes": (_i32, [_vp, _i32]),
    "mvrt_pt_join": (_i32, [_vp, _vp]),
    "mvrt_pt_resolve": (_i32, [_vp, _vp]),
    "mvrt_pt_to_image_async": (_i32, [_vp, _vp, _vp]),
    "mvrt_pt_get_steps": (_i32, [_vp]),
    "mvrt_pt_get_number_of_voxels": (_u64, [_vp]),
    "mvrt_pt_get_octree_bytes": (_u64, [_vp]),
    "mvrt_pt_read_framebuffer": (_i32, [_vp, _vp, _vp]),
    "mvrt_pt_framebuffer_dev": (_vp, [_vp]),
    "mvrt_pt_framebuffer_u8_dev": (_vp, [_vp]),
    "mvrt_pt_set_aovs": (_i32, [_vp, _i32]),
    "mvrt_pt_aov_dev": (_vp, [_vp, _i32]),
    "mvrt_pt_read_aov": (_i32, [_vp, _vp, _i32, _vp]),
    "mvrt_pt_set_moments": (_i32, [_vp, _i32]),
    "mvrt_pt_moments_dev": (_vp, [_vp]),
    "mvrt_pt_read_moments": (_i32, [_vp, _vp, _vp]),
    "mvrt_denoise_default_params": (_i32, [_vp]),
    "mvrt_denoise_scratch_bytes": (_u64, [_i32, _i32]),
    "mvrt_denoise_buffers": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _u64, _vp]),
    "mvrt_pt_denoise": (_i32, [_vp, _vp, _vp]),
    "mvrt_pt_denoised_dev": (_vp, [_vp]),
    "mvrt_pt_read_denoised": (_i32, [_vp, _vp, _vp]),
    "mvrt_pt_set_sample_mask": (_i32, [_vp, _vp, _vp, _vp]),
    "mvrt_pt_active_pixels": (_u64, [_vp]),
    "mvrt_pt_error_mask": (_i32, [_vp, _vp, _f32, _f32, _i32, _i32, _vp, _vp]),
    "mvrt_pt_set_tile": (_i32, [_vp, _i32, _i32]),
    "mvrt_pt_owned_pixels": (_u64, [_vp]),
    "mvrt_pt_assemble_tiles": (_i32, [_vp, _i32, _u64, _i32, _i32, _vp, _vp]),
    "mvrt_resolve_buffer": (_i32, [_vp, _u64, _vp, _vp]),
    "mvrt_pt_sample_radiance_dev": (_vp, [_vp]),
    "mvrt_pt_read_sample_radiance": (_i32, [_vp, _vp, _u64]),
    "mvrt_pt_set_debug_capture": (_i32, [_vp, _i32]),
    "mvrt_pt_read_debug_stage": (_i32, [_vp, _i32, _vp, _u64, _vp]),
    "mvrt_pt_set_test_free_bytes": (_i32, [_vp, _u64]),
    "mvrt_test_fail_allocation": (_i32, [C.c_int64]),
    "mvrt_test_allocation_state": (_i32, [_vp, _vp, _vp]),
    "mvrt_test_ball_stats": (_i32, [_vp]),
    "mvrt_test_enclosed_nearest_stats": (_i32, [_vp]),
    "mvrt_test_nearest_query_stats": (_i32, [_vp]),
    "mvrt_test_resample_stats": (_i32, [_vp]),
    "mvrt_test_peak_bytes": (_i32, [_vp, _i32]),
    "mvrt_pt_set_profiling": (_i32, [_vp, _i32]),
    "mvrt_pt_reset_stats": (_i32, [_vp]),
    "mvrt_pt_get_stats": (_i32, [_vp, _vp, _vp]),
}

_lib = None


def lib():
    """Load libmvrt_hip.so (once).  Raises MvrtError if the HIP library is absent -- no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MvrtError("libmvrt_hip.so is not built (%s); run `python -m massivevoxelraytracing_amd.build`. "
                            "There is no CPU fallback for the GPU path." % LIB_PATH)
        try:
            l = C.CDLL(LIB_PATH)
        except OSError as e:
            raise MvrtError("cannot load %s: %s" % (LIB_PATH, e))
        for name, (res, args) in SIGNATURES.items():
            f = getattr(l, name)
            f.restype = res
            f.argtypes = args
        _lib = l
    return _lib


def _check(rc):
    if rc != 0:
        raise MvrtError(lib().mvrt_last_error().decode("utf-8", "replace"))


def _hp(a):
    """host pointer of a numpy array (or None)"""
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def device_count():
    n = C.c_int(0)
    _check(lib().mvrt_device_count(C.byref(n)))
    return n.value


def set_device(i):
    _check(lib().mvrt_set_device(int(i)))


def device_name():
    buf = C.create_string_buffer(256)
    _check(lib().mvrt_device_name(buf, 256))
    return buf.value.decode()


def synchronize():
    _check(lib().mvrt_device_synchronize())


def set_test_fail_allocation(nth):
    """failure-path tests: the nth device allocation the library makes from now on this thread fails, then the hook is off again (0 = off)"""
    _check(lib().mvrt_test_fail_allocation(int(nth)))


def peak_bytes(reset=False):
    """measuring: the most bytes of device memory the library held at one time since the last reset (mvrt_test_peak_bytes)"""
    v = C.c_uint64(0)
    _check(lib().mvrt_test_peak_bytes(C.byref(v), int(bool(reset))))
    return v.value


def ball_stats():
    """measuring: what the last distance band this thread ran did: {records: per pass along x, y, z, seeds, cells} (mvrt_test_ball_stats)"""
    v = (C.c_uint64 * 5)()
    _check(lib().mvrt_test_ball_stats(v))
    return {"records": [int(v[0]), int(v[1]), int(v[2])], "seeds": int(v[3]), "cells": int(v[4])}


def enclosed_nearest_stats():
    """measuring: what the last enclosed_nearest / fill_enclosed_nearest this thread ran did: {cells, gaps: per pass along x, y, z, longest: the longest gap per
    axis in cells, deepest: the largest d2}; a call that ran no pass leaves all but cells at 0 (mvrt_test_enclosed_nearest_stats)"""
    v = (C.c_uint64 * 8)()
    _check(lib().mvrt_test_enclosed_nearest_stats(v))
    return {"cells": int(v[0]), "gaps": [int(v[1]), int(v[2]), int(v[3])], "longest": [int(v[4]), int(v[5]), int(v[6])], "deepest": int(v[7])}


def nearest_query_stats():
    """measuring: what the last nearest_voxels / nearest_between / transfer_attributes this thread ran did: {queries, visits: the node visits in total, most: the
    most visits of one query, compared: the voxels whose distance was taken} (mvrt_test_nearest_query_stats)"""
    v = (C.c_uint64 * 4)()
    _check(lib().mvrt_test_nearest_query_stats(v))
    return {"queries": int(v[0]), "visits": int(v[1]), "most": int(v[2]), "compared": int(v[3])}


def resample_stats():
    """measuring: what the last resampling this thread ran did: {levels of the destination grid, frontier: the nodes kept per level 1 .. levels, the last entry
    being the result cells} (mvrt_test_resample_stats)"""
    v = (C.c_uint64 * 24)()
    _check(lib().mvrt_test_resample_stats(v))
    return {"levels": int(v[0]), "frontier": [int(v[l]) for l in range(1, int(v[0]) + 1)]}


def cell_transform_from_world(world, src_lower, src_dps, dst_lower, dst_dps):
    """mvrt_cell_transform_from_world: the CellTransform that aligns two lattices in world space.  world: 3x4 row-major (or 12 numbers), p_dst = W p_src + w;
    the lattices by their lower corner (3 float32) and dps.  Host only, no GPU call."""
    w = np.ascontiguousarray(world, np.float64).reshape(12)
    sl, dl = np.ascontiguousarray(src_lower, np.float32).reshape(3), np.ascontiguousarray(dst_lower, np.float32).reshape(3)
    out = CellTransform()
    _check(lib().mvrt_cell_transform_from_world(_hp(w), _hp(sl), float(np.float32(src_dps)), _hp(dl), float(np.float32(dst_dps)), C.byref(out)))
    return out


def allocation_state():
    """(buffers held, bytes held, allocations attempted so far) of the library's own device memory, process-wide"""
    v = [C.c_uint64(0) for _ in range(3)]
    _check(lib().mvrt_test_allocation_state(*[C.byref(x) for x in v]))
    return tuple(x.value for x in v)


class DeviceArray:
    """A typed device buffer owned through mvrt_malloc/mvrt_free (hipUtil.hpp:48-74 'Buffer')."""

    def __init__(self, shape, dtype):
        self.shape = (shape,) if np.isscalar(shape) else tuple(shape)
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        p = C.c_void_p(0)
        _check(lib().mvrt_malloc(C.byref(p), self.nbytes))
        self.ptr = p.value

    @classmethod
    def from_host(cls, a):
        a = np.ascontiguousarray(a)
        d = cls(a.shape, a.dtype)
        if d.nbytes:
            _check(lib().mvrt_memcpy_h2d(d.ptr, _hp(a), d.nbytes, None))
        return d

    def to_host(self):
        out = np.empty(self.shape, self.dtype)
        if self.nbytes:
            _check(lib().mvrt_memcpy_d2h(_hp(out), self.ptr, self.nbytes, None))
        return out

    def free(self):
        if getattr(self, "ptr", None):
            lib().mvrt_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _dev_ptr(x):
    """Accept DeviceArray, raw int pointers or anything with data_ptr() (torch tensors)."""
    if x is None:
        return None
    if isinstance(x, DeviceArray):
        return x.ptr
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    return int(x)


def ao_directions(samples):
    """mvrt_ao_directions: the (6, samples, 3) float32 table of occlusion ray directions, direction d in the order of surface_masks, sample k at the Hammersley
    point ((k + 0.5) / samples, radical inverse of k).  Host only, no GPU call."""
    samples = int(samples)
    out = np.zeros((6, max(samples, 0), 3), np.float32)
    _check(lib().mvrt_ao_directions(samples, _hp(out)))
    return out


def camera_from_matrices(view, proj, focus=1.0, lens_r=0.0):
    """CameraPinhole::initFromPerspective (renderCommon.hpp:21-35); matrices column-major."""
    view = np.ascontiguousarray(view, np.float32).reshape(16)
    proj = np.ascontiguousarray(proj, np.float32).reshape(16)
    cam = np.zeros(15, np.float32)
    _check(lib().mvrt_camera_from_matrices(_hp(view), _hp(proj), focus, lens_r, _hp(cam)))
    return cam


class IntersectorOctreeGPU:
    """reference IntersectorOctreeGPU.hpp:21-275 (host side) + batch form of its device methods."""

    def __init__(self, _borrowed=None):
        self._own = _borrowed is None
        if self._own:
            h = C.c_void_p(0)
            _check(lib().mvrt_svo_create(C.byref(h)))
            self._h = h.value
        else:
            self._h = _borrowed

    def cleanUp(self):
        if self._own and getattr(self, "_h", None):
            lib().mvrt_svo_destroy(self._h)
            self._h = None

    __del__ = cleanUp

    BUILD_NO_DAG = 1
    BUILD_NO_EMBEDDED_MASK = 2
    BUILD_CONSERVATIVE = 4
    SURFACE_MERGE_ANY_ATTRIBUTE = SURFACE_MERGE_ANY_ATTRIBUTE
    SURFACE_MERGE_WELD = SURFACE_MERGE_WELD

    def build_synthetic(self, gridRes, n_random_voxels, seed, origin=(0.0, 0.0, 0.0), dps=None, flags=0, stream=None):
        """seeded random-voxel octree built on the GPU (HBM-bound stress, mvrt_svo_build_synthetic)"""
        o = np.ascontiguousarray(origin, np.float32)
        dps = np.float32(1.0 / gridRes) if dps is None else np.float32(dps)
        _check(lib().mvrt_svo_build_synthetic(self._h, int(gridRes), int(n_random_voxels), int(seed), _hp(o), float(dps), int(flags), stream))

    def build(self, vertices, vcolors, vemissions, stream, origin, dps, gridRes, flags=0):
        """IntersectorOctreeGPU::build(vertices, vcolors, vemissions, Shader*, stream, origin, dps, gridRes)
        (:40-47; the Shader* argument has no counterpart -- kernels are precompiled)."""
        v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
        c = None if vcolors is None else np.ascontiguousarray(vcolors, np.float32).reshape(-1, 3)
        e = None if vemissions is None else np.ascontiguousarray(vemissions, np.float32).reshape(-1, 3)
        o = np.ascontiguousarray(origin, np.float32)
        _check(lib().mvrt_svo_build_ex(self._h, _hp(v), _hp(c), _hp(e), len(v), stream, _hp(o), float(np.float32(dps)), int(gridRes), int(flags)))

    VOXEL_REMOVE = 0
    VOXEL_SET = 1

    @staticmethod
    def _voxel_arrays(xyz, attribs, ops):
        """numpy arrays are copied to the device; DeviceArray (or raw device pointers / torch tensors with data_ptr()) are passed as they are.
        Returns (n, keep-alive list, xyz ptr, attribs ptr, ops ptr)."""
        keep = []

        def dev(a, dtype, width):
            if a is None:
                return None, None
            if isinstance(a, np.ndarray):
                a = np.ascontiguousarray(a, dtype).reshape(-1, width) if width > 1 else np.ascontiguousarray(a, dtype).reshape(-1)
                d = DeviceArray.from_host(a)
                keep.append(d)
                return d.ptr, len(a)
            if isinstance(a, DeviceArray):
                return a.ptr, a.nbytes // (np.dtype(dtype).itemsize * width)
            return _dev_ptr(a), None

        px, n = dev(xyz, np.uint32, 3)
        if n is None:
            raise ValueError("xyz must be a numpy array or a DeviceArray (the entry count is taken from it)")
        pa, na = dev(None if attribs is None else (np.ascontiguousarray(attribs).view(np.uint8).reshape(-1, 8) if isinstance(attribs, np.ndarray) else attribs), np.uint8, 8)
        po, no = dev(ops, np.uint8, 1)
        for m, what in ((na, "attribs"), (no, "ops")):
            if m is not None and m != n:
                raise ValueError("%s has %d entries, xyz %d" % (what, m, n))
        return n, keep, px, pa, po

    def _counts(self, fn, args, n, stream):
        """the call every wrapper that returns counts makes: fn(handle, *args, n uint64 out-counters, stream), checked; -> the count (n == 1) or the n of them"""
        out = [C.c_uint64(0) for _ in range(n)]
        _check(fn(self._h, *args, *[C.byref(c) for c in out], stream))
        return out[0].value if n == 1 else tuple(c.value for c in out)

    @staticmethod
    def _listing(device, lead, outs, stream, scalars=()):
        """a listing in host form.  device = the bound *_device method, device(*lead, capacity, *arrays, stream) -> the count or (count, further counts...);
        outs = ((key, trailing shape, dtype), ...) in the order of its arrays.  The sizing call, one device array of `count` entries per output, the filling call
        unless the count is 0, the copies back; -> {key: host array, ..., then the further counts of the sizing call under the names `scalars`}"""
        r = device(*lead, stream=stream)
        n, more = (r[0], r[1:]) if isinstance(r, tuple) else (r, ())
        arrays = [DeviceArray((n,) + shape, dtype) for _, shape, dtype in outs]
        if n:
            device(*lead, n, *arrays, stream)
        out = {key: a.to_host() for (key, _, _), a in zip(outs, arrays)}
        out.update(zip(scalars, more))
        return out

    _XYZ, _ATTRIBS = ("xyz", (3,), np.uint32), ("attribs", (8,), np.uint8)  # the two outputs most listings share

    def build_voxels(self, xyz, attribs=None, origin=(0.0, 0.0, 0.0), dps=None, gridRes=None, flags=0, stream=None):
        """mvrt_svo_build_voxels: xyz (n, 3) uint32 in [0, gridRes), attribs (n, 8) uint8 VoxelAttirb {color, emission} or None (white, no emission).
        Duplicates merge like the reference's unique (integer mean).  flags: BUILD_NO_DAG | BUILD_NO_EMBEDDED_MASK."""
        n, keep, px, pa, _ = self._voxel_arrays(xyz, attribs, None)
        o = np.ascontiguousarray(origin, np.float32)
        dps = np.float32(1.0 / gridRes) if dps is None else np.float32(dps)
        _check(lib().mvrt_svo_build_voxels(self._h, px, pa, n, _hp(o), float(dps), int(gridRes), int(flags), stream))

    def edit_voxels(self, xyz, attribs=None, ops=None, stream=None):
        """mvrt_svo_edit_voxels: ops per entry VOXEL_SET (1) / VOXEL_REMOVE (0), None = all SET; the last entry per voxel wins."""
        n, keep, px, pa, po = self._voxel_arrays(xyz, attribs, ops)
        _check(lib().mvrt_svo_edit_voxels(self._h, px, pa, po, n, stream))

    def read_voxels(self, stream=None):
        """mvrt_svo_read_voxels -> (xyz (n, 3) uint32, attribs (n, 8) uint8), sorted by Morton code (= vIndex order)"""
        n = self.info().numberOfVoxels
        xyz, at = DeviceArray((n, 3), np.uint32), DeviceArray((n, 8), np.uint8)
        _check(lib().mvrt_svo_read_voxels(self._h, xyz.ptr, at.ptr, stream))
        return xyz.to_host(), at.to_host()

    def walk_voxels_device(self, capacity=0, xyz=None, vIndex=None, attribs=None, stream=None):
        """mvrt_svo_walk_voxels into caller device arrays of `capacity` entries (any may be None; all None = the sizing call); returns the path count.
        On MvrtError nothing was written."""
        return self._counts(lib().mvrt_svo_walk_voxels, (int(capacity), _dev_ptr(xyz), _dev_ptr(vIndex), _dev_ptr(attribs)), 1, stream)

    def walk_voxels(self, stream=None):
        """the voxels of whatever octree the handle holds, uploaded or built, one per root-to-voxel path in ascending path (Morton) order:
        {xyz (n, 3) uint32, vIndex (n,) uint32 = what a trace reports for the voxel, attribs (n, 8) uint8 = the attribute of that vIndex}"""
        return self._listing(self.walk_voxels_device, (), (self._XYZ, ("vIndex", (), np.uint32), self._ATTRIBS), stream)

    def rebuild(self, flags=0, stream=None):
        """mvrt_svo_rebuild: the octree becomes the one build_voxels would build from its walked voxels (attribute bytes and hasEmission kept), after which
        read_voxels / edit_voxels / surface_* accept an upload.  flags: BUILD_NO_DAG | BUILD_NO_EMBEDDED_MASK.  Invalidates device_view() snapshots."""
        _check(lib().mvrt_svo_rebuild(self._h, int(flags), stream))

    def enclosed_cells_device(self, capacity=0, xyz=None, region=None, stream=None):
        """mvrt_svo_enclosed_cells into caller device arrays of `capacity` cells (either may be None; both None = the sizing call); returns (nCells, nRegions).
        On MvrtError nothing was written."""
        return self._counts(lib().mvrt_svo_enclosed_cells, (int(capacity), _dev_ptr(xyz), _dev_ptr(region)), 2, stream)

    def enclosed_cells(self, stream=None):
        """the empty cells no 6-connected path of empty cells joins to the grid border: {xyz (n, 3) uint32 in ascending Morton order, region (n,) uint32 numbered
        by first appearance in that order, nRegions}"""
        return self._listing(self.enclosed_cells_device, (), (self._XYZ, ("region", (), np.uint32)), stream, ("nRegions",))

    def fill_enclosed(self, attrib=None, stream=None):
        """mvrt_svo_fill_enclosed: every enclosed cell becomes a voxel with `attrib` (8 bytes VoxelAttirb {color, emission}; None = white, no emission), exactly
        as edit_voxels would set them; returns the number of cells filled (0: the handle was not touched).  Invalidates device_view() snapshots otherwise."""
        a = None if attrib is None else np.ascontiguousarray(attrib).view(np.uint8).reshape(8)
        return self._counts(lib().mvrt_svo_fill_enclosed, (_hp(a),), 1, stream)

    def enclosed_nearest_device(self, capacity=0, xyz=None, region=None, dist2=None, nearest=None, attribs=None, stream=None):
        """mvrt_svo_enclosed_nearest into caller device arrays of `capacity` cells (any may be None; all None = the sizing call, which runs no distance pass);
        returns (nCells, nRegions).  On MvrtError nothing was written."""
        return self._counts(lib().mvrt_svo_enclosed_nearest, (int(capacity), _dev_ptr(xyz), _dev_ptr(region), _dev_ptr(dist2), _dev_ptr(nearest), _dev_ptr(attribs)), 2, stream)

    def enclosed_nearest(self, stream=None):
        """the enclosed cells of enclosed_cells(), in its order, with their nearest voxel: {xyz (n, 3) uint32, region (n,) uint32, dist2 (n,) uint32 = the exact
        squared distance to the set (no radius; below 2^20), nearest (n,) uint32 = the lowest vIndex among the voxels at that distance, attribs (n, 8) uint8 = that
        voxel's colour and emission with alpha 255, nRegions}"""
        outs = (self._XYZ, ("region", (), np.uint32), ("dist2", (), np.uint32), ("nearest", (), np.uint32), self._ATTRIBS)
        return self._listing(self.enclosed_nearest_device, (), outs, stream, ("nRegions",))

    def fill_enclosed_nearest(self, stream=None):
        """mvrt_svo_fill_enclosed_nearest: every enclosed cell becomes a voxel with the colour and emission of its nearest voxel (taken on the set before the
        fill), exactly as edit_voxels would set the cells and attribs of enclosed_nearest(); returns the number of cells filled (0: the handle was not touched).
        Invalidates device_view() snapshots otherwise."""
        return self._counts(lib().mvrt_svo_fill_enclosed_nearest, (), 1, stream)

    def coarse_voxels_device(self, levels_down, min_count=1, capacity=0, xyz=None, attribs=None, count=None, stream=None):
        """mvrt_svo_coarse_voxels into caller device arrays of `capacity` cells (any may be None; all None = the sizing call); returns the number of kept cells.
        On MvrtError nothing was written."""
        return self._counts(lib().mvrt_svo_coarse_voxels, (int(levels_down), int(min_count), int(capacity), _dev_ptr(xyz), _dev_ptr(attribs), _dev_ptr(count)), 1, stream)

    def coarse_voxels(self, levels_down, min_count=1, stream=None):
        """the voxel set `levels_down` levels coarser: the cells (x >> k, y >> k, z >> k) that hold at least min_count voxels, in ascending Morton order:
        {xyz (n, 3) uint32 coarse coordinates, attribs (n, 8) uint8 = the integer mean per channel with alpha 255, count (n,) uint32 fine voxels per cell}"""
        return self._listing(self.coarse_voxels_device, (levels_down, min_count), (self._XYZ, self._ATTRIBS, ("count", (), np.uint32)), stream)

    def coarsen(self, levels_down, min_count=1, flags=0, dst=None, stream=None):
        """mvrt_svo_coarsen: dst (None = this object, the in-place LOD) becomes the octree build_voxels would build from coarse_voxels() at gridRes >> levels_down
        with `flags` (BUILD_NO_DAG | BUILD_NO_EMBEDDED_MASK), same lower and upper bounds, dps * 2^levels_down.  Returns dst.  Invalidates device_view()
        snapshots of dst."""
        dst = self if dst is None else dst
        _check(lib().mvrt_svo_coarsen(self._h, dst._h, int(levels_down), int(min_count), int(flags), stream))
        return dst

    def dilation_cells_device(self, element=MORPH_CUBE, capacity=0, xyz=None, attribs=None, count=None, stream=None):
        """mvrt_svo_dilation_cells into caller device arrays of `capacity` cells (any may be None; all None = the sizing call); returns the number of cells.
        On MvrtError nothing was written."""
        return self._counts(lib().mvrt_svo_dilation_cells, (int(element), int(capacity), _dev_ptr(xyz), _dev_ptr(attribs), _dev_ptr(count)), 1, stream)

    def dilation_cells(self, element=MORPH_CUBE, stream=None):
        """the cells one dilation step with `element` (MORPH_FACES / MORPH_CUBE) adds, in ascending Morton order: {xyz (n, 3) uint32, attribs (n, 8) uint8 = the
        integer mean per channel over the occupied in-grid neighbours with alpha 255, count (n,) uint32 = their number}"""
        return self._listing(self.dilation_cells_device, (element,), (self._XYZ, self._ATTRIBS, ("count", (), np.uint32)), stream)

    def erosion_voxels_device(self, element=MORPH_CUBE, capacity=0, vIndex=None, stream=None):
        """mvrt_svo_erosion_voxels into a caller device array of `capacity` entries (None = the sizing call); returns the number of voxels a step removes."""
        return self._counts(lib().mvrt_svo_erosion_voxels, (int(element), int(capacity), _dev_ptr(vIndex)), 1, stream)

    def erosion_voxels(self, element=MORPH_CUBE, stream=None):
        """the vIndex, ascending, of the voxels one erosion step removes: those with an empty e-neighbour inside the grid (outside counts as occupied)"""
        return self._listing(self.erosion_voxels_device, (element,), (("vIndex", (), np.uint32),), stream)["vIndex"]

    def dilate(self, element=MORPH_CUBE, steps=1, stream=None):
        """mvrt_svo_dilate: `steps` dilation steps in place, the levels built once; returns the cells added (0: the handle was not touched).  Invalidates
        device_view() snapshots otherwise, like edit_voxels."""
        return self._counts(lib().mvrt_svo_dilate, (int(element), int(steps)), 1, stream)

    def erode(self, element=MORPH_CUBE, steps=1, stream=None):
        """mvrt_svo_erode: `steps` erosion steps in place (outside the grid counts as occupied); returns the voxels removed.  Refused when none would be left."""
        return self._counts(lib().mvrt_svo_erode, (int(element), int(steps)), 1, stream)

    def close(self, element=MORPH_CUBE, steps=1, stream=None):
        """mvrt_svo_close: `steps` dilation steps, then `steps` erosion steps, in place; returns the net cells added.  close(MORPH_CUBE, 1) before fill_enclosed
        repairs a shell with one-voxel holes."""
        return self._counts(lib().mvrt_svo_close, (int(element), int(steps)), 1, stream)

    def open(self, element=MORPH_CUBE, steps=1, stream=None):
        """mvrt_svo_open: `steps` erosion steps, then `steps` dilation steps, in place; a pure removal (the voxels left keep their bytes); returns the net voxels
        removed.  Refused when none would be left."""
        return self._counts(lib().mvrt_svo_open, (int(element), int(steps)), 1, stream)

    def distance_cells_device(self, radius2=1, capacity=0, xyz=None, dist2=None, nearest=None, attribs=None, stream=None):
        """mvrt_svo_distance_cells into caller device arrays of `capacity` cells (any may be None; all None = the sizing call); returns the number of cells.
        On MvrtError nothing was written."""
        return self._counts(lib().mvrt_svo_distance_cells, (int(radius2), int(capacity), _dev_ptr(xyz), _dev_ptr(dist2), _dev_ptr(nearest), _dev_ptr(attribs)), 1, stream)

    def distance_cells(self, radius2=1, stream=None):
        """the empty in-grid cells within squared distance `radius2` (1..1024) of the set, in ascending Morton order: {xyz (n, 3) uint32, dist2 (n,) uint32 = the
        exact squared distance to the set, nearest (n,) uint32 = the lowest vIndex among the voxels at that distance, attribs (n, 8) uint8 = that voxel's colour and
        emission with alpha 255}"""
        return self._listing(self.distance_cells_device, (radius2,), (self._XYZ, ("dist2", (), np.uint32), ("nearest", (), np.uint32), self._ATTRIBS), stream)

    def depth_voxels_device(self, radius2=1, capacity=0, vIndex=None, depth2=None, stream=None):
        """mvrt_svo_depth_voxels into caller device arrays of `capacity` entries (any may be None; both None = the sizing call); returns the number of voxels."""
        return self._counts(lib().mvrt_svo_depth_voxels, (int(radius2), int(capacity), _dev_ptr(vIndex), _dev_ptr(depth2)), 1, stream)

    def depth_voxels(self, radius2=1, stream=None):
        """the voxels whose squared distance to the nearest empty in-grid cell is at most `radius2` (outside the grid counts as occupied), the ones erode_ball
        removes: {vIndex (n,) uint32 ascending, depth2 (n,) uint32}"""
        return self._listing(self.depth_voxels_device, (radius2,), (("vIndex", (), np.uint32), ("depth2", (), np.uint32)), stream)

    def dilate_ball(self, radius2=1, stream=None):
        """mvrt_svo_dilate_ball: the set grown by the ball of squared radius `radius2` in place, one operation, the levels built once; a new cell takes the
        attribute of its nearest voxel.  Returns the cells added (0: the handle was not touched).  Invalidates device_view() snapshots otherwise."""
        return self._counts(lib().mvrt_svo_dilate_ball, (int(radius2),), 1, stream)

    def erode_ball(self, radius2=1, stream=None):
        """mvrt_svo_erode_ball: the voxels deeper than `radius2` stay (outside the grid counts as occupied); returns the voxels removed.  Refused when none would
        be left."""
        return self._counts(lib().mvrt_svo_erode_ball, (int(radius2),), 1, stream)

    def close_ball(self, radius2=1, stream=None):
        """mvrt_svo_close_ball: dilate_ball, then erode_ball, in one call; returns the net cells added."""
        return self._counts(lib().mvrt_svo_close_ball, (int(radius2),), 1, stream)

    def open_ball(self, radius2=1, stream=None):
        """mvrt_svo_open_ball: erode_ball, then dilate_ball, in one call; a pure removal (the voxels left keep their bytes); returns the net voxels removed.
        Refused when none would be left."""
        return self._counts(lib().mvrt_svo_open_ball, (int(radius2),), 1, stream)

    def components_device(self, element=MORPH_CUBE, label=None, capacity=0, size=None, first=None, box=None, stream=None):
        """mvrt_svo_components into caller device arrays: label of numberOfVoxels uint32, size / first of `capacity` uint32, box of capacity x 6 uint32 (any may be
        None; all None = the sizing call); returns (nComponents, largest).  On MvrtError nothing was written."""
        return self._counts(lib().mvrt_svo_components, (int(element), _dev_ptr(label), int(capacity), _dev_ptr(size), _dev_ptr(first), _dev_ptr(box)), 2, stream)

    def components(self, element=MORPH_CUBE, stream=None):
        """the connected components under `element` (MORPH_FACES = 6-connected, MORPH_CUBE = 26-connected), numbered in order of first appearance in vIndex
        order: {label (numberOfVoxels,) uint32, size (n,) uint32, first (n,) uint32 = the lowest vIndex, box (n, 6) uint32 = min x, y, z, max x, y, z}"""
        n, _ = self.components_device(element, stream=stream)
        label, size, first, box = DeviceArray(self.info().numberOfVoxels, np.uint32), DeviceArray(n, np.uint32), DeviceArray(n, np.uint32), DeviceArray((n, 6), np.uint32)
        self.components_device(element, label, n, size, first, box, stream)  # (made at n == 0 too, and label is sized by the voxels: not a _listing)
        return {"label": label.to_host(), "size": size.to_host(), "first": first.to_host(), "box": box.to_host()}

    def keep_components(self, element=MORPH_CUBE, min_voxels=1, keep_largest=0, stream=None):
        """mvrt_svo_keep_components: keeps, in place, the components of at least `min_voxels` voxels and, where keep_largest != 0, only the keep_largest largest
        of them (a tie goes to the component that appears first); exactly edit_voxels with VOXEL_REMOVE on the rest.  Returns (voxels removed, components
        kept); 0 removed: the handle was not touched.  Refused when no voxel would be left."""
        return self._counts(lib().mvrt_svo_keep_components, (int(element), int(min_voxels), int(keep_largest)), 2, stream)

    @staticmethod
    def _offset(offset):
        return None if offset is None else np.ascontiguousarray(offset, np.int32).reshape(3)

    def combine_voxels_device(self, b, op, offset=None, flags=0, capacity=0, xyz=None, attribs=None, source=None, stream=None):
        """mvrt_svo_combine_voxels into caller device arrays of `capacity` voxels (any may be None; all None = the sizing call); returns (n, overlap, clipped).
        On MvrtError nothing was written."""
        return self._counts(lib().mvrt_svo_combine_voxels, (b._h, int(op), _hp(self._offset(offset)), int(flags), int(capacity), _dev_ptr(xyz), _dev_ptr(attribs), _dev_ptr(source)),
                            3, stream)

    def combine_voxels(self, b, op, offset=None, flags=0, stream=None):
        """this set `op` (COMBINE_UNION / _INTERSECTION / _DIFFERENCE / _XOR) the set of `b` moved by `offset` (3 ints, None = 0) and clipped to this grid, in
        ascending Morton order: {xyz (n, 3) uint32, attribs (n, 8) uint8, source (n,) uint8 = 1 this only, 2 b only, 3 both, overlap = the voxels in both,
        clipped = the voxels of b the offset moves out of the grid}.  A voxel of this set keeps its bytes (COMBINE_ATTRIB_B: the overlap takes b's), one of b
        alone takes b's colour and emission with alpha 255.  Neither octree is modified."""
        return self._listing(self.combine_voxels_device, (b, op, offset, flags), (self._XYZ, self._ATTRIBS, ("source", (), np.uint8)), stream, ("overlap", "clipped"))

    def combine(self, b, op, offset=None, flags=0, stream=None):
        """mvrt_svo_combine: this octree becomes combine_voxels(b, op, offset, flags), exactly as edit_voxels with the added voxels (and, under COMBINE_ATTRIB_B,
        the overlap) as VOXEL_SET and the dropped ones as VOXEL_REMOVE would leave it; b may be this object.  Returns (added, removed, clipped); a call that
        changes nothing leaves the handle untouched.  Refused when no voxel would be left.  Invalidates device_view() snapshots otherwise."""
        return self._counts(lib().mvrt_svo_combine, (b._h, int(op), _hp(self._offset(offset)), int(flags)), 3, stream)

    def nearest_voxels_device(self, n, query, max_dist2=NO_LIMIT, dist2=None, nearest=None, attribs=None, stream=None):
        """mvrt_svo_nearest_voxels: n queries (n x 3 int32 on the device) into caller device arrays (dist2 uint64, nearest uint32, attribs 8 bytes per query; any
        may be None).  On MvrtError nothing was written."""
        _check(lib().mvrt_svo_nearest_voxels(self._h, int(n), _dev_ptr(query), int(max_dist2), _dev_ptr(dist2), _dev_ptr(nearest), _dev_ptr(attribs), stream))

    def nearest_voxels(self, query, max_dist2=NO_LIMIT, stream=None):
        """the nearest voxel of every point of `query` ((n, 3) int32 lattice points, each coordinate in [-2^22, 2^22], inside the grid or not), in its order:
        {dist2 (n,) uint64 = the exact squared distance to the set, nearest (n,) uint32 = the lowest vIndex among the voxels at that distance, attribs (n, 8) uint8
        = that voxel's colour and emission with alpha 255}.  A query further than max_dist2 (NO_LIMIT = none, 0 = the membership test) reports NO_LIMIT,
        0xFFFFFFFF and zero bytes.  The octree is not modified."""
        q = np.ascontiguousarray(query, np.int32).reshape(-1, 3)
        if len(q) and (q.min() < -(1 << 22) or q.max() > (1 << 22)):
            raise ValueError("a query coordinate is outside [-2^22, 2^22]")
        n = len(q)
        self.nearest_voxels_device(0, None, max_dist2, stream=stream)  # (what the handle decides is refused before anything is allocated)
        qd = DeviceArray.from_host(q)
        d2, near, at = DeviceArray(n, np.uint64), DeviceArray(n, np.uint32), DeviceArray((n, 8), np.uint8)
        self.nearest_voxels_device(n, qd, max_dist2, d2, near, at, stream)  # (made for n == 0 too; the C++ mirror skips it there)
        return {"dist2": d2.to_host(), "nearest": near.to_host(), "attribs": at.to_host()}

    def nearest_between_device(self, b, offset=None, max_dist2=NO_LIMIT, capacity=0, dist2=None, nearest=None, stream=None):
        """mvrt_svo_nearest_between into caller device arrays of `capacity` entries (either may be None; both None = the summary call); returns {n, maxDist2,
        farthest, zero, beyond}.  On MvrtError nothing was written."""
        n, md, nz, nb, far = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
        _check(lib().mvrt_svo_nearest_between(self._h, b._h, _hp(self._offset(offset)), int(max_dist2), int(capacity), _dev_ptr(dist2), _dev_ptr(nearest), C.byref(n), C.byref(md),
                                              C.byref(far), C.byref(nz), C.byref(nb), stream))
        return {"n": n.value, "maxDist2": md.value, "farthest": far.value, "zero": nz.value, "beyond": nb.value}

    def nearest_between(self, b, offset=None, max_dist2=NO_LIMIT, stream=None):
        """for every voxel v of this set, in vIndex order, the nearest voxel of `b` to v - offset (3 ints, None = 0) in b's cell space: {dist2 (n,) uint64,
        nearest (n,) uint32 = a vIndex of b, n, maxDist2 = the largest dist2 within the limit (the squared one-sided Hausdorff distance from this set to b +
        offset), farthest = the lowest vIndex of this set that attains it, zero = the voxels at distance 0, beyond = the voxels beyond max_dist2}.  Neither octree
        is modified; b may be this object."""
        n = self.info().numberOfVoxels
        if n == 0:
            return self.nearest_between_device(b, offset, max_dist2, stream=stream)  # (an empty handle: the call refuses it)
        d2, near = DeviceArray(n, np.uint64), DeviceArray(n, np.uint32)
        r = self.nearest_between_device(b, offset, max_dist2, n, d2, near, stream)
        r["dist2"], r["nearest"] = d2.to_host(), near.to_host()
        return r

    def transfer_attributes(self, src, offset=None, max_dist2=NO_LIMIT, flags=TRANSFER_COLOUR | TRANSFER_EMISSION, stream=None):
        """mvrt_svo_transfer_attributes: every voxel v of this octree with a voxel of `src` within max_dist2 of v - offset takes the colour (TRANSFER_COLOUR)
        and / or the emission (TRANSFER_EMISSION) of the nearest one, exactly as edit_voxels with VOXEL_SET would store them; the others keep their 8 bytes.
        near is taken before anything is written: src may be this object.  Returns (changed, beyond); a call that changes no byte leaves the handle untouched."""
        return self._counts(lib().mvrt_svo_transfer_attributes, (src._h, _hp(self._offset(offset)), int(max_dist2), int(flags)), 2, stream)

    def resample_voxels_device(self, xf, gridRes=None, capacity=0, xyz=None, attribs=None, source=None, stream=None):
        """mvrt_svo_resample_voxels into caller device arrays of `capacity` voxels (any may be None; all None = the sizing call); returns the count.  gridRes: the
        destination grid (None = this octree's).  On MvrtError nothing was written."""
        res = int((self.info().gridRes or 2) if gridRes is None else gridRes)  # (an empty handle has no grid: the call itself refuses it, "no octree")
        return self._counts(lib().mvrt_svo_resample_voxels, (C.byref(xf), res, int(capacity), _dev_ptr(xyz), _dev_ptr(attribs), _dev_ptr(source)), 1, stream)

    def resample_voxels(self, xf, gridRes=None, stream=None):
        """this set resampled onto a grid of gridRes cells per axis (None = its own) under the CellTransform xf, the INVERSE map from destination cells to source
        cells: the destination cells whose centre maps into a voxel, in ascending Morton order: {xyz (n, 3) uint32, attribs (n, 8) uint8 = that voxel's colour and
        emission with alpha 255, source (n,) uint32 = its vIndex}.  The octree is not modified."""
        return self._listing(self.resample_voxels_device, (xf, gridRes), (self._XYZ, self._ATTRIBS, ("source", (), np.uint32)), stream)

    def resample(self, xf, dst=None, origin=None, dps=None, gridRes=None, flags=0, stream=None):
        """mvrt_svo_resample: dst (None = this object) becomes the octree build_voxels would build from resample_voxels(xf, gridRes) with origin, dps, gridRes (None
        = this octree's own lattice) and `flags` (BUILD_NO_DAG | BUILD_NO_EMBEDDED_MASK).  Returns dst.  Refused when no voxel would be left.  Invalidates
        device_view() snapshots of dst."""
        dst = self if dst is None else dst
        i = self.info() if origin is None or dps is None or gridRes is None else None
        o = np.ascontiguousarray(i.lower[:] if origin is None else origin, np.float32).reshape(3)
        dps = np.float32(i.dps if dps is None else dps)
        res = int((i.gridRes or 2) if gridRes is None else gridRes)
        self._counts(lib().mvrt_svo_resample, (dst._h, C.byref(xf), _hp(o), float(dps), res, int(flags)), 1, stream)
        return dst

    def surface_masks_device(self, masks_dev=None, stream=None):
        """mvrt_svo_surface_masks into a caller's device array of numberOfVoxels bytes (None = count only); returns nFaces"""
        return self._counts(lib().mvrt_svo_surface_masks, (_dev_ptr(masks_dev),), 1, stream)

    def surface_masks(self, stream=None):
        """mvrt_svo_surface_masks -> (masks (numberOfVoxels,) uint8 in vIndex order, nFaces): bit d of a mask = the neighbour in direction d is empty,
        d = 0 -Y, 1 +Y, 2 -Z, 3 +X, 4 +Z, 5 -X"""
        masks = DeviceArray(self.info().numberOfVoxels, np.uint8)
        n = self.surface_masks_device(masks, stream)
        return masks.to_host(), n

    def surface_exterior_masks_device(self, masks_dev=None, stream=None):
        """mvrt_svo_surface_exterior_masks into a caller's device array of numberOfVoxels bytes (None = counts only); returns (nFaces, nHidden): the exterior
        faces and the faces of surface_masks that look into an enclosed cell.  The octree is not modified."""
        return self._counts(lib().mvrt_svo_surface_exterior_masks, (_dev_ptr(masks_dev),), 2, stream)

    def surface_exterior_masks(self, stream=None):
        """mvrt_svo_surface_exterior_masks -> (masks (numberOfVoxels,) uint8 in vIndex order, nFaces, nHidden): the masks of surface_masks without the bits that
        look into an enclosed cell -- the masks the same voxels have after fill_enclosed"""
        masks = DeviceArray(self.info().numberOfVoxels, np.uint8)
        nf, nh = self.surface_exterior_masks_device(masks, stream)
        return masks.to_host(), nf, nh

    @staticmethod
    def _given_masks(masks):
        """masks= of the surface calls: a numpy uint8 array goes to the device, a device array is passed on"""
        return DeviceArray.from_host(np.ascontiguousarray(masks, np.uint8)) if isinstance(masks, np.ndarray) else masks

    def surface_quads_device(self, face_capacity=0, faceVoxel=None, faceDir=None, positions=None, stream=None, *, masks=None):
        """mvrt_svo_surface_quads into caller device arrays (any may be None; all None = the sizing call); returns nFaces.  On MvrtError nothing was written.
        masks (numberOfVoxels uint8, numpy or device): mvrt_svo_surface_quads_masked, the faces are the set bits 0..5 of the masks as given."""
        args = (int(face_capacity), _dev_ptr(faceVoxel), _dev_ptr(faceDir), _dev_ptr(positions))
        if masks is None:
            return self._counts(lib().mvrt_svo_surface_quads, args, 1, stream)
        m = self._given_masks(masks)
        return self._counts(lib().mvrt_svo_surface_quads_masked, (_dev_ptr(m),) + args, 1, stream)

    def surface_quads(self, stream=None, *, masks=None):
        """the exposed faces as unwelded quads: {faceVoxel (n,) uint32 vIndex, faceDir (n,) uint8, positions (n, 4, 3) float32}, faces by vIndex then direction;
        masks: the faces of the given masks instead (surface_quads_device)"""
        masks = None if masks is None else self._given_masks(masks)
        n = self.surface_quads_device(stream=stream, masks=masks)
        fv, fd, pos = DeviceArray(n, np.uint32), DeviceArray(n, np.uint8), DeviceArray((n, 4, 3), np.float32)
        self.surface_quads_device(n, fv, fd, pos, stream, masks=masks)  # (the surface listings make the filling call at a count of 0 too)
        return {"faceVoxel": fv.to_host(), "faceDir": fd.to_host(), "positions": pos.to_host()}

    def surface_mesh_device(self, face_capacity=0, vertex_capacity=0, faceVoxel=None, faceDir=None, indices=None, vertices=None, stream=None, *, masks=None):
        """mvrt_svo_surface_mesh into caller device arrays (any may be None; all None = the sizing call); returns (nFaces, nVertices).
        masks: mvrt_svo_surface_mesh_masked (surface_quads_device)"""
        args = (int(face_capacity), int(vertex_capacity), _dev_ptr(faceVoxel), _dev_ptr(faceDir), _dev_ptr(indices), _dev_ptr(vertices))
        if masks is None:
            return self._counts(lib().mvrt_svo_surface_mesh, args, 2, stream)
        m = self._given_masks(masks)
        return self._counts(lib().mvrt_svo_surface_mesh_masked, (_dev_ptr(m),) + args, 2, stream)

    def surface_mesh(self, stream=None, *, masks=None):
        """the exposed faces over shared vertices: {vertices (m, 3) float32 in corner-key order, indices (n, 4) uint32, faceVoxel (n,), faceDir (n,)};
        masks: the faces of the given masks instead (surface_quads_device)"""
        masks = None if masks is None else self._given_masks(masks)
        nf, nv = self.surface_mesh_device(stream=stream, masks=masks)
        fv, fd, idx, vtx = DeviceArray(nf, np.uint32), DeviceArray(nf, np.uint8), DeviceArray((nf, 4), np.uint32), DeviceArray((nv, 3), np.float32)
        self.surface_mesh_device(nf, nv, fv, fd, idx, vtx, stream, masks=masks)
        return {"vertices": vtx.to_host(), "indices": idx.to_host(), "faceVoxel": fv.to_host(), "faceDir": fd.to_host()}

    def surface_merged_device(self, flags=0, rect_capacity=0, vertex_capacity=0, rectVoxel=None, rectDir=None, rectSize=None, positions=None, indices=None, vertices=None,
                              stream=None, *, masks=None):
        """mvrt_svo_surface_merged into caller device arrays (any may be None; all None = the sizing call); returns (nFaces, nRects, nVertices).
        flags: SURFACE_MERGE_ANY_ATTRIBUTE | SURFACE_MERGE_WELD; indices / vertices need the weld flag.  On MvrtError nothing was written.
        masks: mvrt_svo_surface_merged_masked (surface_quads_device)"""
        args = (int(flags), int(rect_capacity), int(vertex_capacity)) + tuple(_dev_ptr(a) for a in (rectVoxel, rectDir, rectSize, positions, indices, vertices))
        if masks is None:
            return self._counts(lib().mvrt_svo_surface_merged, args, 3, stream)
        m = self._given_masks(masks)
        return self._counts(lib().mvrt_svo_surface_merged_masked, (_dev_ptr(m),) + args, 3, stream)

    def surface_merged(self, flags=0, stream=None, *, masks=None):
        """the exposed faces merged into rectangles, ascending (direction, plane, u0, v0): {nFaces, rectVoxel (n,) uint32 the anchor's vIndex, rectDir (n,) uint8,
        rectSize (n, 2) uint32 (du, dv), positions (n, 4, 3) float32}; with SURFACE_MERGE_WELD also {vertices (m, 3) float32, indices (n, 4) uint32};
        masks: the faces of the given masks instead (surface_quads_device)"""
        masks = None if masks is None else self._given_masks(masks)
        nf, nr, nv = self.surface_merged_device(flags, stream=stream, masks=masks)
        weld = bool(flags & self.SURFACE_MERGE_WELD)
        rv, rd, rs, pos = DeviceArray(nr, np.uint32), DeviceArray(nr, np.uint8), DeviceArray((nr, 2), np.uint32), DeviceArray((nr, 4, 3), np.float32)
        idx, vtx = (DeviceArray((nr, 4), np.uint32), DeviceArray((nv, 3), np.float32)) if weld else (None, None)
        self.surface_merged_device(flags, nr, nv, rv, rd, rs, pos, idx, vtx, stream, masks=masks)
        out = {"nFaces": nf, "rectVoxel": rv.to_host(), "rectDir": rd.to_host(), "rectSize": rs.to_host(), "positions": pos.to_host()}
        if weld:
            out.update(vertices=vtx.to_host(), indices=idx.to_host())
        return out

    def surface_smooth_device(self, params=None, face_capacity=0, vertex_capacity=0, faceVoxel=None, faceDir=None, indices=None, vertices=None, displacements=None,
                              neighbours=None, stream=None, *, masks=None):
        """mvrt_svo_surface_smooth into caller device arrays (any may be None; all None = the sizing call, which runs no iteration); returns
        (nFaces, nVertices, clamped).  params: a SmoothParams (None = the defaults); masks: the faces of the given masks (surface_quads_device).
        On MvrtError nothing was written."""
        m = None if masks is None else self._given_masks(masks)
        args = (_dev_ptr(m), None if params is None else C.byref(params), int(face_capacity), int(vertex_capacity)) + tuple(
            _dev_ptr(a) for a in (faceVoxel, faceDir, indices, vertices, displacements, neighbours))
        return self._counts(lib().mvrt_svo_surface_smooth, args, 3, stream)

    def surface_smooth(self, iterations=4, weights=(256, 256), limit=127, stream=None, *, masks=None):
        """the mesh of surface_mesh smoothed by constrained surface nets: {vertices (m, 3) float32, indices (n, 4) uint32, faceVoxel (n,), faceDir (n,),
        displacements (m, 3) int32 in steps of 1/256 cell, neighbours (m,) uint8 (bit 0 -x, 1 +x, 2 -y, 3 +y, 4 -z, 5 +z), clamped}.  weights: (even, odd)
        iterations, 256 = the plain Laplacian step, (128, -136) Taubin's pair; limit <= 127 keeps all vertices apart.  masks: as surface_mesh"""
        p = SmoothParams()
        _check(lib().mvrt_smooth_default_params(C.byref(p)))
        p.iterations, p.weightEven, p.weightOdd, p.limit = int(iterations), int(weights[0]), int(weights[1]), int(limit)
        masks = None if masks is None else self._given_masks(masks)
        nf, nv, _ = self.surface_smooth_device(p, stream=stream, masks=masks)
        fv, fd, idx, vtx = DeviceArray(nf, np.uint32), DeviceArray(nf, np.uint8), DeviceArray((nf, 4), np.uint32), DeviceArray((nv, 3), np.float32)
        disp, nbr = DeviceArray((nv, 3), np.int32), DeviceArray(nv, np.uint8)
        _, _, clamped = self.surface_smooth_device(p, nf, nv, fv, fd, idx, vtx, disp, nbr, stream, masks=masks)
        return {"vertices": vtx.to_host(), "indices": idx.to_host(), "faceVoxel": fv.to_host(), "faceDir": fd.to_host(), "displacements": disp.to_host(),
                "neighbours": nbr.to_host(), "clamped": clamped}

    def upload(self, nodes68, attribs, origin, dps, gridRes, hasEmission=0, embeddedMask=True, stream=None):
        nodes68 = np.ascontiguousarray(nodes68)
        assert nodes68.dtype.itemsize == 68 or nodes68.dtype == np.uint8
        n_nodes = nodes68.nbytes // 68
        attribs = np.ascontiguousarray(attribs, np.uint8).reshape(-1, 8)
        o = np.ascontiguousarray(origin, np.float32)
        _check(lib().mvrt_svo_upload(self._h, _hp(nodes68), n_nodes, _hp(attribs), len(attribs), _hp(o), float(np.float32(dps)), int(gridRes), int(hasEmission),
                                     int(embeddedMask), stream))

    @staticmethod
    def check_upload(nodes68, numberOfVoxels, gridRes, embeddedMask=True):
        """mvrt_svo_check_upload: the upload contract (include/mvrt.h) on host arrays, no GPU call.  Returns None when mvrt_svo_upload would accept
        the octree, else the error text (it names the rule and the first offending node)."""
        nodes68 = np.ascontiguousarray(nodes68)
        assert nodes68.dtype.itemsize == 68 or nodes68.dtype == np.uint8
        if lib().mvrt_svo_check_upload(_hp(nodes68), nodes68.nbytes // 68, int(numberOfVoxels), int(gridRes), int(embeddedMask)) == 0:
            return None
        return lib().mvrt_last_error().decode("utf-8", "replace")

    def info(self):
        i = SvoInfo()
        _check(lib().mvrt_svo_get_info(self._h, C.byref(i)))
        return i

    # reference public fields (:265-274)
    m_numberOfNodes = property(lambda s: s.info().numberOfNodes)
    m_numberOfVoxels = property(lambda s: s.info().numberOfVoxels)
    m_lower = property(lambda s: np.array(s.info().lower[:], np.float32))
    m_upper = property(lambda s: np.array(s.info().upper[:], np.float32))
    m_dps = property(lambda s: s.info().dps)
    m_hasEmission = property(lambda s: s.info().hasEmission)
    m_nodeBuffer = property(lambda s: lib().mvrt_svo_node_buffer_dev(s._h))  # device pointers (:265-266)
    m_vAttributeBuffer = property(lambda s: lib().mvrt_svo_attribute_buffer_dev(s._h))

    def device_view(self):
        """mvrt_svo_device_view: the ctypes DeviceOctree a HIP kernel built on include/mvrt/device.hpp takes by value.
        A snapshot: any later build (build_voxels included) / edit_voxels / upload / cleanUp of this object invalidates it."""
        v = DeviceOctree()
        _check(lib().mvrt_svo_device_view(self._h, C.byref(v)))
        return v

    def traversal_bytes(self):
        return lib().mvrt_svo_traversal_bytes(self._h)

    def hasEmission(self):
        return bool(self.info().hasEmission)

    def set_emission_scale(self, s):
        _check(lib().mvrt_svo_set_emission_scale(self._h, s))

    def download(self, want_morton=False, stream=None):
        from numpy import dtype
        i = self.info()
        nodes = np.zeros(i.numberOfNodes * 68, np.uint8)
        attrs = np.zeros((i.numberOfVoxels, 8), np.uint8)
        morton = np.zeros(i.numberOfVoxels, np.uint64) if want_morton else None
        _check(lib().mvrt_svo_download(self._h, _hp(nodes), _hp(attrs), _hp(morton), stream))
        return nodes, attrs, morton

    def intersect(self, ro, rd, isShadowRay=None, want_descents=False):
        """Batch IntersectorOctreeGPU::intersect (:243-251) on packed host arrays (n,3)."""
        ro = np.ascontiguousarray(ro, np.float32).reshape(-1, 3)
        rd = np.ascontiguousarray(rd, np.float32).reshape(-1, 3)
        n = len(ro)
        sh = None if isShadowRay is None else np.ascontiguousarray(isShadowRay, np.uint8)
        t = np.zeros(n, np.float32)
        nm = np.zeros(n, np.int32)
        vi = np.zeros(n, np.uint32)
        de = np.zeros(n, np.uint32)
        _check(lib().mvrt_trace_batch_host(self._h, n, _hp(ro), _hp(rd), _hp(sh), _hp(t), _hp(nm), _hp(vi), _hp(de)))
        out = {"t": t, "nMajor": nm, "vIndex": vi}
        if want_descents:
            out["descents"] = de
        return out

    def intersect_device(self, n, rox, roy, roz, rdx, rdy, rdz, isShadow, t, nMajor, vIndex, descents=None, stream=None):
        _check(lib().mvrt_trace_batch(self._h, n, *[_dev_ptr(a) for a in (rox, roy, roz, rdx, rdy, rdz, isShadow, t, nMajor, vIndex, descents)], stream))

    def intersect_range(self, ro, rd, tMax, isShadowRay=None, want_descents=False):
        """mvrt_trace_batch_range on packed host arrays (n,3) and one limit per ray (a scalar = the same for all): the hit of intersect() where its t <= tMax, else a miss"""
        ro = np.ascontiguousarray(ro, np.float32).reshape(-1, 3)
        rd = np.ascontiguousarray(rd, np.float32).reshape(-1, 3)
        n = len(ro)
        lim = np.ascontiguousarray(np.broadcast_to(np.asarray(tMax, np.float32), (n,)))
        dev = [DeviceArray.from_host(np.ascontiguousarray(a)) for a in (ro[:, 0], ro[:, 1], ro[:, 2], rd[:, 0], rd[:, 1], rd[:, 2])]
        sh = None if isShadowRay is None else DeviceArray.from_host(np.ascontiguousarray(isShadowRay, np.uint8))
        t, nm, vi, de = DeviceArray(n, np.float32), DeviceArray(n, np.int32), DeviceArray(n, np.uint32), DeviceArray(n, np.uint32)
        dlim = DeviceArray.from_host(lim)
        self.intersect_range_device(n, *dev, sh, dlim, t, nm, vi, de)
        synchronize()
        out = {"t": t.to_host(), "nMajor": nm.to_host(), "vIndex": vi.to_host()}
        if want_descents:
            out["descents"] = de.to_host()
        return out

    def intersect_range_device(self, n, rox, roy, roz, rdx, rdy, rdz, isShadow, tMax, t, nMajor=None, vIndex=None, descents=None, stream=None):
        _check(lib().mvrt_trace_batch_range(self._h, n, *[_dev_ptr(a) for a in (rox, roy, roz, rdx, rdy, rdz, isShadow, tMax, t, nMajor, vIndex, descents)], stream))

    def lod_prepare(self, stream=None):
        """mvrt_svo_lod_prepare: attach the attribute pyramid of the cone-limited rays (per level the cells of coarse_voxels(levels - L, 1)); returns its size in
        bytes.  Every build, edit, rebuild, upload, coarsen in place and cleanUp drops it."""
        _check(lib().mvrt_svo_lod_prepare(self._h, stream))
        return self.lod_bytes()

    def lod_release(self):
        _check(lib().mvrt_svo_lod_release(self._h))

    def lod_bytes(self):
        """mvrt_svo_lod_bytes: the size of the pyramid, 0 without one"""
        return int(lib().mvrt_svo_lod_bytes(self._h))

    def lod_view(self):
        """mvrt_svo_lod_view: the ctypes DeviceLod a HIP kernel built on include/mvrt/device.hpp takes by value.  A snapshot, like device_view()."""
        v = DeviceLod()
        _check(lib().mvrt_svo_lod_view(self._h, C.byref(v)))
        return v

    def lod_level(self, level):
        """level `level` in [1, levels - 1] of the prepared pyramid on the host: {code (n,) uint64, attribs (n, 8) uint8, count (n,) uint32}"""
        v = self.lod_view()
        if not 1 <= level < v.levels:
            raise ValueError("level %d is outside [1, %d]" % (level, v.levels - 1))
        n = v.count[level]
        out = {"code": np.empty(n, np.uint64), "attribs": np.empty((n, 8), np.uint8), "count": np.empty(n, np.uint32)}
        for key, ptr in (("code", v.codes[level]), ("attribs", v.attrs[level]), ("count", v.cellVoxels[level])):
            if n:
                _check(lib().mvrt_memcpy_d2h(_hp(out[key]), ptr, out[key].nbytes, None))
        return out

    def intersect_cone(self, ro, rd, coneA, coneB, want_attribs=False):
        """mvrt_trace_batch_cone on packed host arrays (n,3) and one cone per ray (scalars = the same for all): {t, nMajor, level, cellCode, descents} and, with
        want_attribs (needs lod_prepare), index and attribs (n, 8)"""
        ro = np.ascontiguousarray(ro, np.float32).reshape(-1, 3)
        rd = np.ascontiguousarray(rd, np.float32).reshape(-1, 3)
        n = len(ro)
        dev = [DeviceArray.from_host(np.ascontiguousarray(a)) for a in (ro[:, 0], ro[:, 1], ro[:, 2], rd[:, 0], rd[:, 1], rd[:, 2])]
        dev += [DeviceArray.from_host(np.ascontiguousarray(np.broadcast_to(np.asarray(c, np.float32), (n,)))) for c in (coneA, coneB)]
        t, nm, lv, code, de = DeviceArray(n, np.float32), DeviceArray(n, np.int32), DeviceArray(n, np.uint32), DeviceArray(n, np.uint64), DeviceArray(n, np.uint32)
        idx, at = (DeviceArray(n, np.uint32), DeviceArray((n, 8), np.uint8)) if want_attribs else (None, None)
        self.intersect_cone_device(n, *dev, t, nm, lv, code, idx, at, de)
        synchronize()
        out = {"t": t.to_host(), "nMajor": nm.to_host(), "level": lv.to_host(), "cellCode": code.to_host(), "descents": de.to_host()}
        if want_attribs:
            out.update(index=idx.to_host(), attribs=at.to_host())
        return out

    def intersect_cone_device(self, n, rox, roy, roz, rdx, rdy, rdz, coneA, coneB, t, nMajor=None, level=None, cellCode=None, index=None, attrib=None, descents=None,
                              stream=None):
        _check(lib().mvrt_trace_batch_cone(self._h, n, *[_dev_ptr(a) for a in (rox, roy, roz, rdx, rdy, rdz, coneA, coneB, t, nMajor, level, cellCode, index, attrib,
                                                                                 descents)], stream))

    def render_lod(self, camera, width, height, lodScale, showVertexColor=False, stream=None):
        """mvrt_render_primary_lod: render() with one cone per pixel, lodScale pixels wide; returns host arrays {rgba, t, nMajor, level, descents}.
        showVertexColor needs lod_prepare."""
        cam = np.ascontiguousarray(camera, np.float32)
        n = width * height
        rgba, t, nm, lv, de = DeviceArray((n, 4), np.uint8), DeviceArray(n, np.float32), DeviceArray(n, np.int32), DeviceArray(n, np.uint32), DeviceArray(n, np.uint32)
        _check(lib().mvrt_render_primary_lod(self._h, _hp(cam), width, height, float(np.float32(lodScale)), int(showVertexColor), rgba.ptr, t.ptr, nm.ptr, lv.ptr, de.ptr,
                                             stream))
        _check(lib().mvrt_stream_synchronize(stream))
        return {"rgba": rgba.to_host(), "t": t.to_host(), "nMajor": nm.to_host(), "level": lv.to_host(), "descents": de.to_host()}

    def surface_ao_device(self, nFaces, faceVoxel, faceDir, samples, radius, open, stream=None):
        """mvrt_svo_surface_ao into a caller device array of nFaces uint16: per face the number of `samples` occlusion rays that are open within `radius`.
        On MvrtError nothing was written."""
        _check(lib().mvrt_svo_surface_ao(self._h, int(nFaces), _dev_ptr(faceVoxel), _dev_ptr(faceDir), int(samples), float(np.float32(radius)), _dev_ptr(open), stream))

    def surface_ao(self, samples=64, radius=None, stream=None, *, masks=None):
        """the exposed faces with their baked occlusion: {faceVoxel (n,) uint32, faceDir (n,) uint8, open (n,) uint16 in [0, samples]}; radius defaults to 8 * dps;
        masks: the faces of the given masks instead (surface_quads_device)"""
        if radius is None:
            radius = np.float32(8) * np.float32(self.info().dps)
        masks = None if masks is None else self._given_masks(masks)
        n = self.surface_quads_device(stream=stream, masks=masks)
        fv, fd, op = DeviceArray(n, np.uint32), DeviceArray(n, np.uint8), DeviceArray(n, np.uint16)
        self.surface_quads_device(n, fv, fd, None, stream, masks=masks)
        self.surface_ao_device(n, fv, fd, samples, radius, op, stream)
        return {"faceVoxel": fv.to_host(), "faceDir": fd.to_host(), "open": op.to_host()}

    def intersect_hinted(self, ro, rd, origin_voxel_morton, isShadowRay=None):
        """mvrt_trace_batch_hinted on packed host arrays: per ray the Morton code of an EXISTING voxel (or 2^64-1 = no hint) to start below the root from"""
        ro = np.ascontiguousarray(ro, np.float32).reshape(-1, 3)
        rd = np.ascontiguousarray(rd, np.float32).reshape(-1, 3)
        n = len(ro)
        dev = [DeviceArray.from_host(np.ascontiguousarray(a)) for a in (ro[:, 0], ro[:, 1], ro[:, 2], rd[:, 0], rd[:, 1], rd[:, 2])]
        sh = None if isShadowRay is None else DeviceArray.from_host(np.ascontiguousarray(isShadowRay, np.uint8))
        hint = DeviceArray.from_host(np.ascontiguousarray(origin_voxel_morton, np.uint64))
        t, nm, vi, de = DeviceArray(n, np.float32), DeviceArray(n, np.int32), DeviceArray(n, np.uint32), DeviceArray(n, np.uint32)
        _check(lib().mvrt_trace_batch_hinted(self._h, n, *[_dev_ptr(a) for a in dev], _dev_ptr(sh), hint.ptr, t.ptr, nm.ptr, vi.ptr, de.ptr, None))
        synchronize()
        return {"t": t.to_host(), "nMajor": nm.to_host(), "vIndex": vi.to_host(), "descents": de.to_host()}

    def render(self, camera, width, height, showVertexColor=False, want_hits=True, stream=None):
        """the `render` kernel launch of voxRTGPU.cpp:191-203; returns host arrays"""
        cam = np.ascontiguousarray(camera, np.float32)
        n = width * height
        rgba = DeviceArray((n, 4), np.uint8)
        t = DeviceArray(n, np.float32) if want_hits else None
        nm = DeviceArray(n, np.int32) if want_hits else None
        vi = DeviceArray(n, np.uint32) if want_hits else None
        de = DeviceArray(n, np.uint32) if want_hits else None
        _check(lib().mvrt_render_primary(self._h, _hp(cam), width, height, int(showVertexColor), rgba.ptr, *[_dev_ptr(a) for a in (t, nm, vi, de)], stream))
        _check(lib().mvrt_stream_synchronize(stream))
        out = {"rgba": rgba.to_host()}
        if want_hits:
            out.update(t=t.to_host(), nMajor=nm.to_host(), vIndex=vi.to_host(), descents=de.to_host())
        return out

    def render_device(self, camera, width, height, showVertexColor, rgba_dev, stream=None):
        cam = np.ascontiguousarray(camera, np.float32)
        _check(lib().mvrt_render_primary(self._h, _hp(cam), width, height, int(showVertexColor), _dev_ptr(rgba_dev), None, None, None, None, stream))


def read_rgbe_file(path):
    """host-only: the .hdr decoder behind PathTracer.loadHDRI -> (rgba float32 (h*w, 4), w, h)"""
    w, h = C.c_int(0), C.c_int(0)
    _check(lib().mvrt_rgbe_read_file(path.encode(), None, 0, C.byref(w), C.byref(h)))
    out = np.zeros((w.value * h.value, 4), np.float32)
    _check(lib().mvrt_rgbe_read_file(path.encode(), _hp(out), len(out), C.byref(w), C.byref(h)))
    return out, w.value, h.value


def compact_indices(keep):
    """Stable compaction indices of host flags through the device path (StreamCompaction semantics)."""
    keep = np.ascontiguousarray(keep, np.uint8)
    n = len(keep)
    d_keep = DeviceArray.from_host(keep)
    d_dst = DeviceArray(max(n, 1), np.uint32)
    d_kept = DeviceArray(1, np.uint32)
    _check(lib().mvrt_compact_indices(d_keep.ptr, n, d_dst.ptr, d_kept.ptr, None))
    synchronize()
    return d_dst.to_host()[:n], int(d_kept.to_host()[0])


class PathTracer:
    """reference PathTracer.hpp:14-170.  Same method names and call order; prlib types are replaced by
    plain arrays (camera = 15 floats or view/proj matrices; images = numpy arrays)."""

    def __init__(self):
        h = C.c_void_p(0)
        _check(lib().mvrt_pt_create(C.byref(h)))
        self._h = h.value
        self.m_intersectorOctreeGPU = IntersectorOctreeGPU(_borrowed=lib().mvrt_pt_intersector(self._h))

    def cleanUp(self):
        if getattr(self, "_h", None):
            lib().mvrt_pt_destroy(self._h)
            self._h = None

    __del__ = cleanUp

    def setup(self, stream=None, kernel=None, includeDir=None, isNvidia=False):
        """PathTracer::setup(stream, kernel, includeDir, isNvidia) (:43-69); the last three are ignored."""
        _check(lib().mvrt_pt_setup(self._h, stream))

    def pmj_table(self):
        """PMJSampler::m_samples as the host generated it (128 x 4096 float2)"""
        out = np.zeros(2 * 4096 * 128, np.float32)
        _check(lib().mvrt_pt_download_pmj(self._h, _hp(out)))
        return out

    def set_tile(self, tile_index, tile_count):
        _check(lib().mvrt_pt_set_tile(self._h, tile_index, tile_count))

    def resizeFrameBufferIfNeeded(self, stream, width, height):
        _check(lib().mvrt_pt_resize_framebuffer_if_needed(self._h, stream, width, height))
        self.m_width, self.m_height = width, height

    def clearFrameBuffer(self, stream=None):
        _check(lib().mvrt_pt_clear_framebuffer(self._h, stream))

    def loadHDRI(self, stream, file, filePrimary=None):
        _check(lib().mvrt_pt_load_hdri_file(self._h, stream, file.encode(), None if filePrimary is None else filePrimary.encode()))

    def loadHDRIPixels(self, stream, rgba, w, h, rgbaPrimary=None, wp=0, hp=0):
        rgba = np.ascontiguousarray(rgba, np.float32)
        prim = None if rgbaPrimary is None else np.ascontiguousarray(rgbaPrimary, np.float32)
        _check(lib().mvrt_pt_load_hdri(self._h, stream, _hp(rgba), w, h, _hp(prim), wp, hp))

    def hdri_sat(self, which, w, h):
        out = np.zeros(w * h, np.uint32)
        _check(lib().mvrt_pt_download_hdri_sat(self._h, which, _hp(out)))
        return out

    def set_hdri_scale(self, s):
        _check(lib().mvrt_pt_set_hdri_scale(self._h, s))

    def updateScene(self, vertices, vcolors, vemissions, stream, origin, dps, gridRes):
        self.m_intersectorOctreeGPU.build(vertices, vcolors, vemissions, stream, origin, dps, gridRes)

    def step(self, stream, camera, focus=None, lensR=None):
        """PathTracer::step(stream, camera, focus, lensR) (:150-169).  `camera` is either the 15 CameraPinhole
        floats (focus/lensR already inside) or a (view, proj) pair of column-major 4x4 matrices."""
        if isinstance(camera, (tuple, list)) and len(camera) == 2:
            view = np.ascontiguousarray(camera[0], np.float32).reshape(16)
            proj = np.ascontiguousarray(camera[1], np.float32).reshape(16)
            _check(lib().mvrt_pt_step_matrices(self._h, stream, _hp(view), _hp(proj), focus, lensR))
        else:
            cam = np.array(camera, np.float32, copy=True)
            if focus is not None:
                cam[14] = focus
            if lensR is not None:
                cam[13] = lensR
            _check(lib().mvrt_pt_step(self._h, stream, _hp(cam)))

    def set_batch_steps(self, n):
        _check(lib().mvrt_pt_set_batch_steps(self._h, n))

    def set_split_small_passes(self, enable):
        _check(lib().mvrt_pt_set_split_small_passes(self._h, 1 if enable else 0))

    def set_origin_hints(self, enable):
        _check(lib().mvrt_pt_set_origin_hints(self._h, 1 if enable else 0))

    def set_pipeline_depth(self, depth):
        _check(lib().mvrt_pt_set_pipeline_depth(self._h, depth))

    def join(self, stream=None):
        """make `stream` wait for the steps still in flight on the internal streams"""
        _check(lib().mvrt_pt_join(self._h, stream))

    def resolve(self, stream=None):
        _check(lib().mvrt_pt_resolve(self._h, stream))

    def toImageAsync(self, stream=None, output=None):
        n = self.owned_pixels()
        out = np.zeros((n, 4), np.uint8) if output is None else output
        _check(lib().mvrt_pt_to_image_async(self._h, stream, _hp(out)))
        return out

    def getSteps(self):
        return lib().mvrt_pt_get_steps(self._h)

    def getNumberOfVoxels(self):
        return lib().mvrt_pt_get_number_of_voxels(self._h)

    def getOctreeBytes(self):
        return lib().mvrt_pt_get_octree_bytes(self._h)

    def owned_pixels(self):
        return lib().mvrt_pt_owned_pixels(self._h)

    def read_framebuffer(self, stream=None):
        out = np.zeros((self.owned_pixels(), 4), np.float32)
        _check(lib().mvrt_pt_read_framebuffer(self._h, stream, _hp(out)))
        return out

    def framebuffer_dev(self):
        return lib().mvrt_pt_framebuffer_dev(self._h)

    AOV_ALBEDO = 0        # xyz = sum of the first hit's voxel colour, w = samples whose primary ray hit
    AOV_NORMAL_DEPTH = 1  # xyz = sum of the first hit's axis normal, w = sum of its t

    def set_aovs(self, enable):
        """mvrt_pt_set_aovs: first-hit feature buffers beside the frame buffer (off by default); fails while steps are accumulated"""
        _check(lib().mvrt_pt_set_aovs(self._h, 1 if enable else 0))

    def read_aov(self, which, stream=None):
        """(owned_pixels, 4) host copy of one feature buffer; means are sum / read_framebuffer()[:, 3]"""
        out = np.zeros((self.owned_pixels(), 4), np.float32)
        _check(lib().mvrt_pt_read_aov(self._h, stream, int(which), _hp(out)))
        return out

    def aov_dev(self, which):
        """device pointer of one feature buffer, None when they are off (join() before reading it on a stream of your own)"""
        return lib().mvrt_pt_aov_dev(self._h, int(which))

    def set_moments(self, enable):
        """mvrt_pt_set_moments: per-pixel sums of the samples' luminance and of its square beside the frame buffer (off by default); fails while steps are accumulated"""
        _check(lib().mvrt_pt_set_moments(self._h, 1 if enable else 0))

    def read_moments(self, stream=None):
        """(owned_pixels, 4) host copy: x = sum of l, y = sum of l * l, z = w = 0"""
        out = np.zeros((self.owned_pixels(), 4), np.float32)
        _check(lib().mvrt_pt_read_moments(self._h, stream, _hp(out)))
        return out

    def moments_dev(self):
        """device pointer of the moments, None when they are off (join() before reading it on a stream of your own)"""
        return lib().mvrt_pt_moments_dev(self._h)

    def denoise(self, stream=None, **params):
        """mvrt_pt_denoise: filter the accumulated frame into the handle's denoised buffer (needs set_aovs, set_moments, one tile, >= 1 step).
        params: fields of mvrt_denoise_params (iterations, sigmaNormal, sigmaDepth, sigmaCoverage, sigmaLuminance, albedoFloor, flags) over the defaults"""
        _check(lib().mvrt_pt_denoise(self._h, stream, C.byref(denoise_params(**params)) if params else None))

    def read_denoised(self, stream=None):
        """(width * height, 4) host copy of the denoised buffer: xyz = mean radiance, w = 1"""
        out = np.zeros((self.m_width * self.m_height, 4), np.float32)
        _check(lib().mvrt_pt_read_denoised(self._h, stream, _hp(out)))
        return out

    def denoised_dev(self):
        """device pointer of the denoised buffer; None before the first denoise and after a resize"""
        return lib().mvrt_pt_denoised_dev(self._h)

    def set_sample_mask(self, mask, stream=None):
        """mvrt_pt_set_sample_mask: the steps that follow sample only the owned pixels whose byte is nonzero; None = every pixel again.  `mask`: a numpy array
        (one entry per owned pixel, or per valid owned pixel: the padding is filled with 0) or a device array of owned_pixels() bytes.  Returns the number of
        active pixels.  clearFrameBuffer, a reallocating resize and set_tile drop the mask"""
        n = C.c_uint64(0)
        if mask is None:
            _check(lib().mvrt_pt_set_sample_mask(self._h, stream, None, C.byref(n)))
            return n.value
        dev = mask
        if isinstance(mask, np.ndarray):
            host = np.zeros(self.owned_pixels(), np.uint8)
            flat = np.asarray(mask).reshape(-1) != 0
            if len(flat) > len(host):
                raise MvrtError("set_sample_mask: %d mask entries for %d owned pixels" % (len(flat), len(host)))
            host[: len(flat)] = flat
            dev = DeviceArray.from_host(host)
        _check(lib().mvrt_pt_set_sample_mask(self._h, stream, _dev_ptr(dev), C.byref(n)))  # (blocks: the temporary copy may go)
        return n.value

    def active_pixels(self):
        """the pixels a step samples: the valid owned pixels when no mask is set, 0 without a frame"""
        return lib().mvrt_pt_active_pixels(self._h)

    def error_mask(self, threshold, lum_floor=0.01, min_samples=32, max_samples=0, out_dev=None, stream=None):
        """mvrt_pt_error_mask: 1 where the standard error of the pixel's mean luminance exceeds threshold * max( mean, lum_floor ) or the pixel has fewer than
        min_samples samples, 0 from max_samples on (0 = no limit); needs set_moments.  Returns (mask, count): mask = out_dev when given (a device array of
        owned_pixels() bytes, nothing is copied back), else an (owned_pixels,) uint8 host array.  Sets no mask: pass the result to set_sample_mask"""
        n = C.c_uint64(0)
        dev = out_dev
        if dev is None and self.owned_pixels():
            dev = DeviceArray(self.owned_pixels(), np.uint8)
        # (without a frame there is nothing to size an array by: the library refuses the call on the host before it looks at the pointer)
        ptr = _dev_ptr(dev) if dev is not None else C.c_void_p(1)
        _check(lib().mvrt_pt_error_mask(self._h, stream, float(threshold), float(lum_floor), int(min_samples), int(max_samples), ptr, C.byref(n)))
        return (out_dev if out_dev is not None else dev.to_host()), n.value

    def sample_radiance(self, n_samples=None):
        """per-sample radiance of the last pass: (n, 3) host array (debug / parity)"""
        n = self.owned_pixels() * 16 if n_samples is None else n_samples
        out = np.zeros((3, n), np.float32)
        _check(lib().mvrt_pt_read_sample_radiance(self._h, _hp(out), n))
        return out.T.copy()

    def set_debug_capture(self, on):
        _check(lib().mvrt_pt_set_debug_capture(self._h, int(on)))

    def debug_stage_survivors(self, stage, capacity=None):
        """sample ids of the paths that survived shade stage `stage` of the last pass, in compacted-slot order (needs set_debug_capture)"""
        cap = self.owned_pixels() * 16 * 8 if capacity is None else capacity
        out = np.zeros(cap, np.uint32)
        n = C.c_uint32(0)
        _check(lib().mvrt_pt_read_debug_stage(self._h, stage, _hp(out), cap, C.byref(n)))
        return out[: n.value].copy()

    def set_test_free_bytes(self, nbytes):
        """failure-path tests: budget the path state against `nbytes` of free HBM (0 = what the device reports)"""
        _check(lib().mvrt_pt_set_test_free_bytes(self._h, int(nbytes)))

    def set_profiling(self, on):
        _check(lib().mvrt_pt_set_profiling(self._h, int(on)))

    def reset_stats(self):
        _check(lib().mvrt_pt_reset_stats(self._h))

    def stats(self, stream=None):
        s = PtStats()
        _check(lib().mvrt_pt_get_stats(self._h, stream, C.byref(s)))
        return {k: getattr(s, k) for k, _ in PtStats._fields_}


def memcpy_d2d(dst_dev, src_dev, nbytes, stream=None):
    _check(lib().mvrt_memcpy_d2d(_dev_ptr(dst_dev), _dev_ptr(src_dev), nbytes, stream))


def assemble_tiles(gathered_dev, tile_count, rank_stride_pixels, width, height, frame_dev, stream=None):
    _check(lib().mvrt_pt_assemble_tiles(_dev_ptr(gathered_dev), tile_count, rank_stride_pixels, width, height, _dev_ptr(frame_dev), stream))


def denoise_params(**fields):
    """mvrt_denoise_params: the library's defaults with `fields` set over them"""
    p = DenoiseParams()
    _check(lib().mvrt_denoise_default_params(C.byref(p)))
    for k, v in fields.items():
        if k not in dict(DenoiseParams._fields_) or k == "reserved":
            raise TypeError("mvrt_denoise_params has no field %r" % k)
        setattr(p, k, v)
    return p


def denoise_scratch_bytes(width, height):
    n = lib().mvrt_denoise_scratch_bytes(int(width), int(height))
    if n == 0:
        _check(1)
    return n


def denoise_buffers(color_dev, albedo_dev, normal_depth_dev, moments_dev, width, height, out_dev, scratch_dev=None, scratch_bytes=None, stream=None, **params):
    """mvrt_denoise_buffers on full-frame device buffers (e.g. assembled tile shares).  scratch_dev None: a DeviceArray is allocated for the call and the
    stream is synchronised before it is freed."""
    own = None
    if scratch_dev is None:
        scratch_bytes = denoise_scratch_bytes(width, height)
        own = scratch_dev = DeviceArray(scratch_bytes, np.uint8)
    try:
        _check(lib().mvrt_denoise_buffers(_dev_ptr(color_dev), _dev_ptr(albedo_dev), _dev_ptr(normal_depth_dev), _dev_ptr(moments_dev), int(width), int(height),
                                          C.byref(denoise_params(**params)) if params else None, _dev_ptr(out_dev), _dev_ptr(scratch_dev), int(scratch_bytes), stream))
        if own is not None:
            _check(lib().mvrt_stream_synchronize(stream))
    finally:
        if own is not None:
            own.free()


def resolve_buffer(rgba_f32_dev, n_pixels, rgba_u8_dev, stream=None):
    _check(lib().mvrt_resolve_buffer(_dev_ptr(rgba_f32_dev), n_pixels, _dev_ptr(rgba_u8_dev), stream))
