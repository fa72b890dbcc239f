"""ctypes binding of the MI355X ray-marcher's C ABI (include/vr/vr.h, include/vr/vr_host.h).

Python here is plumbing for tests and the benchmark; the product is lib/libvr_amd.so (HIP
kernels for gfx950 + the C ABI).  The class `OffscreenPass` mirrors the reference's
`Vol::Rendering::OffscreenPass` API (src/rendering/offscreen_pass.h:40-54): same method names,
argument meaning and error behaviour (failures raise RuntimeError, as the reference throws
std::runtime_error).  There is NO CPU fallback: if the shared library is missing this module
raises at import-time use, and every render goes through the HIP kernels.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# VR_AMD_LIB selects an experiment build (make LIBDIR=... EXTRA=...); default: lib/
LIB_PATH = os.environ.get("VR_AMD_LIB") or os.path.join(HERE, "lib", "libvr_amd.so")

# enum vr_dtype
DTYPE_I8, DTYPE_U8, DTYPE_I16, DTYPE_U16, DTYPE_I32, DTYPE_U32 = 1, 2, 3, 4, 5, 6
DTYPE_I64, DTYPE_U64, DTYPE_F32, DTYPE_F64 = 7, 8, 9, 10
NP_TO_DTYPE = {
    np.dtype(np.int8): DTYPE_I8, np.dtype(np.uint8): DTYPE_U8,
    np.dtype(np.int16): DTYPE_I16, np.dtype(np.uint16): DTYPE_U16,
    np.dtype(np.int32): DTYPE_I32, np.dtype(np.uint32): DTYPE_U32,
    np.dtype(np.int64): DTYPE_I64, np.dtype(np.uint64): DTYPE_U64,
    np.dtype(np.float32): DTYPE_F32, np.dtype(np.float64): DTYPE_F64,
}
DTYPE_TO_NP = {v: k for k, v in NP_TO_DTYPE.items()}
STORAGE_BYTES = {0: 1, 1: 1, 2: 2, 3: 2, 4: 4}  # vr::StorageType -> bytes per voxel

OUT_RGBA8, OUT_RGBA32F = 0, 1


class vr_camera(C.Structure):
    _fields_ = [("view", C.c_float * 16), ("position", C.c_float * 3),
                ("fovy_deg", C.c_float), ("znear", C.c_float), ("zfar", C.c_float)]


class vr_params(C.Structure):
    _fields_ = [("step", C.c_float), ("ray_dist", C.c_float), ("ert_eps", C.c_float),
                ("shading", C.c_int32), ("clear_color", C.c_float * 4),
                ("ambient", C.c_float), ("diffuse", C.c_float), ("specular", C.c_float),
                ("spec_power", C.c_int32), ("tile_order", C.c_int32),
                ("skip_empty", C.c_int32), ("wave_shape", C.c_int32),
                ("frames_in_flight", C.c_int32), ("exact_gradient", C.c_int32),
                ("depth_zero_to_one", C.c_int32)]


class vr_stats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("samples", C.c_uint64),
                ("shaded_samples", C.c_uint64), ("steps", C.c_uint64),
                ("skipped_samples", C.c_uint64)]


class vr_orbit_camera(C.Structure):
    _fields_ = [("center", C.c_float * 3), ("orientation", C.c_float * 4),
                ("radius", C.c_float)]


class vr_memory_info(C.Structure):  # vr.h (ABI 7; history fields ABI 9)
    _fields_ = [(n, C.c_uint64) for n in (
        "volume_bytes", "field_bytes", "oblique_copy_bytes", "plain_copy_bytes",
        "stencil_copy_bytes", "skip_bytes", "derived_bytes", "budget_bytes",
        "builds", "evictions", "downgrades", "last_downgrade")]


class vr_dist_host_profile(C.Structure):  # vr_dist.h
    _fields_ = [("frames", C.c_uint64)] + [(n, C.c_double) for n in (
        "render_us", "gather_us", "assemble_us", "record_us", "wait_us", "total_us")]


# vr.h enum vr_derived (vr_memory_info.last_downgrade)
DERIVED = {1: "field", 2: "oblique_copy", 3: "plain_copy", 4: "stencil_copy", 5: "skip",
           6: "ymajor_copy", 7: "ymajor_field"}


class vr_member_timing(C.Structure):  # vr_debug.h (ABI 7)
    _fields_ = [("device", C.c_int32), ("frames", C.c_uint64), ("kernel_ms", C.c_double),
                ("render_ms", C.c_double), ("gather_ms", C.c_double), ("assemble_ms", C.c_double)]


class vr_variant_facts(C.Structure):  # vr_debug.h
    _fields_ = [(n, C.c_int32) for n in (
        "layout", "mode", "shade", "count", "skip", "field", "field_half", "pipeline", "tf_n",
        "pair", "mip_inflight")]


class vr_mpr_plane(C.Structure):  # vr_mpr.h
    _fields_ = [("origin", C.c_float * 3), ("du", C.c_float * 3), ("dv", C.c_float * 3),
                ("dn", C.c_float * 3), ("width", C.c_uint32), ("height", C.c_uint32),
                ("nsamples", C.c_uint32), ("op", C.c_int32)]


class vr_hist_request(C.Structure):  # vr_hist.h
    _fields_ = [("lo", C.c_float), ("hi", C.c_float), ("nbins", C.c_uint32),
                ("use_box", C.c_uint32), ("box_min", C.c_uint32 * 3), ("box_max", C.c_uint32 * 3)]


class vr_hist_info(C.Structure):  # vr_hist.h
    _fields_ = [("voxels", C.c_uint64), ("below", C.c_uint64), ("above", C.c_uint64),
                ("nan", C.c_uint64), ("vmin", C.c_float), ("vmax", C.c_float)]


class vr_hit_request(C.Structure):  # vr_hit.h
    _fields_ = [("kind", C.c_int32), ("threshold", C.c_float), ("use_rect", C.c_uint32),
                ("rect", C.c_uint32 * 4)]


class vr_hit(C.Structure):  # vr_hit.h
    _fields_ = [("pos", C.c_float * 3), ("depth", C.c_float), ("value", C.c_float),
                ("step", C.c_uint32)]


class vr_mesh_request(C.Structure):  # vr_mesh.h
    _fields_ = [("iso", C.c_float), ("closed", C.c_uint32), ("normals", C.c_uint32),
                ("use_box", C.c_uint32), ("box_min", C.c_uint32 * 3), ("box_max", C.c_uint32 * 3)]


class vr_mesh_vertex(C.Structure):  # vr_mesh.h
    _fields_ = [("pos", C.c_float * 3), ("normal", C.c_float * 3)]


class vr_mesh_info(C.Structure):  # vr_mesh.h
    _fields_ = [("vertices", C.c_uint64), ("triangles", C.c_uint64), ("inside_voxels", C.c_uint64),
                ("reserved", C.c_uint64)]


class vr_label_request(C.Structure):  # vr_label.h
    _fields_ = [("lo", C.c_float), ("hi", C.c_float), ("connectivity", C.c_uint32),
                ("use_box", C.c_uint32), ("box_min", C.c_uint32 * 3), ("box_max", C.c_uint32 * 3)]


class vr_label_component(C.Structure):  # vr_label.h
    _fields_ = [("label", C.c_uint32), ("reserved", C.c_uint32), ("voxels", C.c_uint64),
                ("bbox_min", C.c_uint32 * 3), ("bbox_max", C.c_uint32 * 3), ("sum", C.c_uint64 * 3)]


class vr_label_info(C.Structure):  # vr_label.h
    _fields_ = [("voxels", C.c_uint64), ("in_voxels", C.c_uint64), ("components", C.c_uint64),
                ("largest_voxels", C.c_uint64), ("largest_label", C.c_uint32), ("reserved", C.c_uint32)]


class vr_edt_info(C.Structure):  # vr_morph.h
    _fields_ = [("voxels", C.c_uint64), ("target_voxels", C.c_uint64), ("max_dist2", C.c_uint32),
                ("max_index", C.c_uint32)]


class vr_morph_info(C.Structure):  # vr_morph.h
    _fields_ = [("voxels", C.c_uint64), ("in_set", C.c_uint64), ("out_set", C.c_uint64)]


class vr_mask_select_request(C.Structure):  # vr_maskcc.h
    _fields_ = [("rule", C.c_uint32), ("connectivity", C.c_uint32), ("min_voxels", C.c_uint64),
                ("seed", C.c_uint32 * 3), ("reserved", C.c_uint32)]


class vr_mask_select_info(C.Structure):  # vr_maskcc.h
    _fields_ = [("voxels", C.c_uint64), ("in_set", C.c_uint64), ("out_set", C.c_uint64),
                ("components", C.c_uint64), ("kept", C.c_uint64)]


class vr_mstat_region(C.Structure):  # vr_mstat.h
    _fields_ = [("label", C.c_uint32), ("reserved", C.c_uint32), ("voxels", C.c_uint64), ("nan", C.c_uint64),
                ("vmin", C.c_float), ("vmax", C.c_float), ("min_index", C.c_uint32), ("max_index", C.c_uint32),
                ("sum", C.c_double), ("sum2", C.c_double), ("reserved2", C.c_uint64)]


class vr_mstat_info(C.Structure):  # vr_mstat.h
    _fields_ = [("voxels", C.c_uint64), ("set", C.c_uint64), ("unlisted", C.c_uint64), ("regions", C.c_uint64)]


class vr_mview_source(C.Structure):  # vr_mview.h
    _fields_ = [("ext", C.c_uint32 * 3), ("origin", C.c_uint32 * 3), ("elem_bytes", C.c_uint32),
                ("select", C.c_uint32), ("label", C.c_uint32), ("reserved", C.c_uint32),
                ("array", C.c_void_p), ("occupancy", C.c_void_p)]


class vr_mask_hit(C.Structure):  # vr_mview.h
    _fields_ = [("pos", C.c_float * 3), ("depth", C.c_float), ("element", C.c_uint32), ("step", C.c_uint32),
                ("index", C.c_uint32), ("normal", C.c_int8 * 3), ("reserved", C.c_uint8)]


class vr_mview_info(C.Structure):  # vr_mview.h
    _fields_ = [(n, C.c_uint64) for n in ("voxels", "pixels", "covered", "hits", "steps", "samples")]


class vr_mview_occ_info(C.Structure):  # vr_mview.h
    _fields_ = [(n, C.c_uint64) for n in ("voxels", "cells", "cells_set", "matching")]


class vr_mmesh_request(C.Structure):  # vr_mmesh.h
    _fields_ = [("ext", C.c_uint32 * 3), ("origin", C.c_uint32 * 3), ("elem_bytes", C.c_uint32),
                ("select", C.c_uint32), ("label", C.c_uint32), ("closed", C.c_uint32), ("normals", C.c_uint32),
                ("smooth_iters", C.c_uint32), ("relax", C.c_float), ("reserved", C.c_uint32),
                ("array", C.c_void_p)]


class vr_mmesh_info(C.Structure):  # vr_mmesh.h
    _fields_ = [(n, C.c_uint64) for n in ("voxels", "vertices", "triangles", "matching")]


class vr_dataset(C.Structure):
    _fields_ = [("dims", C.c_uint32 * 3), ("dtype", C.c_int), ("data", C.c_void_p),
                ("vmin", C.c_float), ("vmax", C.c_float)]


# Every entry point include/vr/vr.h and include/vr/vr_host.h declare (checked by the CPU tests).
ABI_SYMBOLS = [
    "vr_abi_version", "vr_params_default", "vr_create", "vr_destroy", "vr_last_error",
    "vr_create_mask", "vr_get_device_mask",
    "vr_resize", "vr_get_size", "vr_get_device", "vr_set_volume", "vr_set_volume_device", "vr_generate_volume",
    "vr_volume_bytes", "vr_debug_read_volume", "vr_debug_read_volume_native", "vr_debug_volume_info",
    "vr_set_transfer_function", "vr_set_slicing", "vr_render", "vr_render_device",
    "vr_shard_rows", "vr_assemble_rows", "vr_count_work", "vr_timing_enable",
    "vr_timing_read", "vr_timing_reset", "vr_kernel_name",
    "vr_import_memory_fd", "vr_release_external_memory",
    "vr_set_row_share", "vr_get_row_share", "vr_shard_rows_ctx",
    "vr_set_memory_budget", "vr_memory_report", "vr_prepare",
]
HOST_SYMBOLS = [
    "vr_cam_init", "vr_cam_rotate", "vr_cam_zoom", "vr_cam_position", "vr_cam_view",
    "vr_cam_to_camera", "vr_gradient_create", "vr_gradient_destroy",
    "vr_gradient_add_color_marker", "vr_gradient_add_alpha_marker",
    "vr_gradient_remove_color_marker", "vr_gradient_remove_alpha_marker",
    "vr_gradient_set_alpha_marker", "vr_gradient_set_color_marker", "vr_gradient_marker_count",
    "vr_gradient_sample", "vr_gradient_discretize", "vr_nrrd_load", "vr_nrrd_write_raw",
    "vr_csv_load", "vr_dataset_free", "vr_host_last_error", "vr_mesh_write_ply",
]

DIST_SYMBOLS = [
    "vr_dist_unique_id", "vr_dist_create", "vr_dist_render", "vr_dist_synchronize",
    "vr_dist_last_error", "vr_dist_destroy", "vr_dist_timing_enable", "vr_dist_timing_read",
    "vr_dist_host_profile_enable", "vr_dist_host_profile_read",
]
DIST_ID_BYTES = 128  # include/vr/vr_dist.h VR_DIST_ID_BYTES
DEBUG_SYMBOLS = ["vr_debug_set_knob", "vr_debug_get_knob", "vr_debug_timing_member",
                 "vr_debug_create_members", "vr_debug_fail_member",
                 "vr_debug_host_profile_enable", "vr_debug_host_profile_member",
                 "vr_debug_variant_name", "vr_debug_last_kernel_name", "vr_debug_label_pass_ms",
                 "vr_debug_ymajor_copy_bytes", "vr_debug_ymajor_field_bytes"]
# include/vr/vr_modes.h: render modes (context state) and enum vr_render_mode
MODES_SYMBOLS = ["vr_set_render_mode", "vr_get_render_mode"]
MODE_COMPOSITE, MODE_MIP = 0, 1
MODE_ISO = 3  # (2 is unassigned and refused)
MODE_MINIP, MODE_MEAN = 4, 6  # minimum- and mean-intensity projection (5 is unassigned and refused)
# include/vr/vr_iso.h: the isovalue of VR_MODE_ISO (context state)
ISO_SYMBOLS = ["vr_set_isovalue", "vr_get_isovalue"]
# include/vr/vr_mpr.h: multi-planar reformat (its own entry points, no render mode) and enum vr_mpr_op
MPR_SYMBOLS = ["vr_mpr_render", "vr_mpr_render_device", "vr_mpr_count_work", "vr_mpr_axis_plane"]
OP_MAX, OP_MIN, OP_MEAN = 0, 1, 2
MPR_MAX_SAMPLES = 4096
AXIS_SAGITTAL, AXIS_CORONAL, AXIS_AXIAL = 0, 1, 2
# include/vr/vr_hist.h: the volume's value histogram, a percentile window, the window setter
HIST_SYMBOLS = ["vr_histogram", "vr_hist_edges", "vr_hist_window", "vr_set_value_range"]
HIST_MAX_BINS = 4096
# include/vr/vr_hit.h: per-pixel hit records of the 3D frame, picking, and enum vr_hit_kind
HIT_SYMBOLS = ["vr_hit_render", "vr_hit_render_device", "vr_hit_count_work", "vr_pick"]
HIT_ENTRY, HIT_OPACITY, HIT_MAX, HIT_MIN, HIT_ISO = 0, 1, 2, 3, 4
HIT_DTYPE = np.dtype([("pos", "<f4", 3), ("depth", "<f4"), ("value", "<f4"), ("step", "<u4")])
HIT_MISS_STEP = 0xFFFFFFFF
# include/vr/vr_mesh.h: the isosurface as an indexed triangle mesh (surface nets on the device)
MESH_SYMBOLS = ["vr_mesh_count", "vr_mesh_extract", "vr_mesh_extract_device"]
MESH_VERTEX_DTYPE = np.dtype([("pos", "<f4", 3), ("normal", "<f4", 3)])
ENOSPC = -28  # VR_ENOSPC
# include/vr/vr_label.h: connected components of a value window and seeded region growing
LABEL_SYMBOLS = ["vr_label_count", "vr_label_components", "vr_label_components_device",
                 "vr_region_grow", "vr_region_grow_device"]
LABEL_COMPONENT_DTYPE = np.dtype([("label", "<u4"), ("reserved", "<u4"), ("voxels", "<u8"),
                                  ("bbox_min", "<u4", 3), ("bbox_max", "<u4", 3), ("sum", "<u8", 3)])
# include/vr/vr_morph.h: the exact distance transform of a mask and ball morphology; the entry points
# live in a second library, lib/libvr_amd_morph.so (morph_lib()), on the same context
MORPH_SYMBOLS = ["vr_edt_squared", "vr_edt_squared_device", "vr_mask_morph", "vr_mask_morph_device",
                 "vr_morph_last_kernel_name"]
EDT_NONE = 0xFFFFFFFF
EDT_TO_SET, EDT_TO_UNSET = 0, 1
MORPH_DILATE, MORPH_ERODE, MORPH_OPEN, MORPH_CLOSE = 0, 1, 2, 3
MORPH_MAX_EXTENT = 32768
# include/vr/vr_maskcc.h: the components of a mask -- labels, records, selection and hole filling; the
# entry points live in a third library, lib/libvr_amd_maskcc.so (maskcc_lib()), on the same context
MASKCC_SYMBOLS = ["vr_mask_label", "vr_mask_label_device", "vr_mask_select", "vr_mask_select_device",
                  "vr_maskcc_last_kernel_name"]
MASK_KEEP_LARGEST, MASK_KEEP_MIN_VOXELS, MASK_KEEP_SEED, MASK_FILL_HOLES = 0, 1, 2, 3
MASKCC_MAX_EXTENT = 32768
# include/vr/vr_mstat.h: the statistics of the volume under a mask or a label array and the value-window
# pass; the entry points live in a fourth library, lib/libvr_amd_mstat.so (mstat_lib()), on the same context
MSTAT_SYMBOLS = ["vr_mask_stats", "vr_mask_stats_device", "vr_label_stats", "vr_label_stats_device",
                 "vr_mask_window", "vr_mask_window_device", "vr_mstat_last_kernel_name"]
MSTAT_REGION_DTYPE = np.dtype([("label", "<u4"), ("reserved", "<u4"), ("voxels", "<u8"), ("nan", "<u8"),
                               ("vmin", "<f4"), ("vmax", "<f4"), ("min_index", "<u4"), ("max_index", "<u4"),
                               ("sum", "<f8"), ("sum2", "<f8"), ("reserved2", "<u8")])
MSTAT_NONE = 0xFFFFFFFF
MSTAT_MAX_EXTENT = 32768
# include/vr/vr_mview.h: the view of a mask or a label array -- first-hit records, the slice's elements, the
# pick and the occupancy words; the entry points live in a fifth library, lib/libvr_amd_mview.so
# (mview_lib()), on the same context
MVIEW_SYMBOLS = ["vr_mview_occupancy_words", "vr_mask_occupancy_device", "vr_mask_hit_render_device",
                 "vr_mask_hit_render", "vr_mask_pick", "vr_mask_slice_device", "vr_mask_slice",
                 "vr_mview_last_kernel_name"]
MVIEW_HIT_DTYPE = np.dtype([("pos", "<f4", 3), ("depth", "<f4"), ("element", "<u4"), ("step", "<u4"),
                            ("index", "<u4"), ("normal", "i1", 3), ("reserved", "u1")])
MVIEW_ANY, MVIEW_LABEL = 0, 1
MVIEW_MISS = 0xFFFFFFFF
MVIEW_CELL = 8
MVIEW_MAX_EXTENT = 32768
# include/vr/vr_mmesh.h: the surface of a mask, or of one label of a label array, as a triangle mesh
# with optional cell-constrained smoothing; the entry points live in a sixth library,
# lib/libvr_amd_mmesh.so (mmesh_lib()), on the same context
MMESH_SYMBOLS = ["vr_mask_mesh_count_device", "vr_mask_mesh_count", "vr_mask_mesh_extract_device",
                 "vr_mask_mesh_extract", "vr_mmesh_last_kernel_name"]
MMESH_MAX_ITERS = 64
MMESH_MAX_EXTENT = 32768
# include/vr/vr_debug.h enum vr_exchange (multi-device contexts: how shards reach member 0)
EXCHANGE_RCCL, EXCHANGE_COPY = 0, 1
# include/vr/vr_debug.h enum vr_knob (launch-policy overrides: speed only, never results)
KNOBS = {"pipeline": 1, "pair": 2, "pair_lanes": 3, "grad_field": 4, "u8_layout": 6,
         "tile_order": 7, "narrow": 8, "alt_geometry": 9, "mip_inflight": 10, "field_order": 11,
         "hist_agg": 12, "hit_inflight": 13}
KNOB_AUTO = {"pipeline": -1, "pair": -1, "pair_lanes": 0, "grad_field": -1,
             "u8_layout": -1, "tile_order": 0, "narrow": 1, "alt_geometry": -1,
             "mip_inflight": 0, "field_order": -1, "hist_agg": -1,
             "hit_inflight": -1}

ABI_VERSION = 9  # include/vr/vr.h VR_ABI_VERSION
_LIB = None


def lib() -> C.CDLL:
    """Load lib/libvr_amd.so (fails loudly: there is no fallback path)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `make -C volumetric-renderer_amd` "
                           "(or __graft_entry__.build()); there is no CPU fallback")
    # PyTorch ships its own libamdhip64.so.7 / libhsa-runtime64.so.1 under the same sonames as
    # /opt/rocm's.  Whichever loads first serves the whole process, and torch's CUDA init
    # failed ("No HIP GPUs are available") once this library had brought in /opt/rocm's
    # runtime and initialised it.  Load torch first when it is installed, so the process
    # runs one runtime that both use (the one the GPU tests and bench.py run on).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, u32, f32, i32 = C.c_void_p, C.c_uint32, C.c_float, C.c_int
    sig = {
        "vr_abi_version": (i32, []),
        "vr_params_default": (None, [C.POINTER(vr_params)]),
        "vr_create": (vp, [i32, u32, u32]),
        "vr_destroy": (None, [vp]),
        "vr_last_error": (C.c_char_p, [vp]),
        "vr_resize": (i32, [vp, u32, u32]),
        "vr_get_size": (i32, [vp, C.POINTER(u32), C.POINTER(u32)]),
        "vr_get_device": (i32, [vp, C.POINTER(i32)]),
        "vr_create_mask": (vp, [u32, u32, u32]),
        "vr_get_device_mask": (i32, [vp, C.POINTER(u32)]),
        "vr_dist_unique_id": (i32, [vp]),
        "vr_dist_create": (vp, [vp, vp, i32, i32, u32, i32]),
        "vr_dist_render": (i32, [vp, C.POINTER(vr_camera), C.POINTER(vr_params), vp, vp]),
        "vr_dist_synchronize": (i32, [vp]),
        "vr_dist_last_error": (C.c_char_p, [vp]),
        "vr_dist_destroy": (None, [vp]),
        "vr_dist_timing_enable": (i32, [vp, i32]),
        "vr_dist_host_profile_enable": (i32, [vp, i32]),
        "vr_dist_host_profile_read": (i32, [vp, C.POINTER(vr_dist_host_profile)]),
        "vr_dist_timing_read": (i32, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                      C.POINTER(C.c_uint64)]),
        "vr_set_volume": (i32, [vp, vp, i32, u32, u32, u32, f32, f32]),
        "vr_set_volume_device": (i32, [vp, vp, i32, u32, u32, u32, f32, f32, vp]),
        "vr_generate_volume": (i32, [vp, i32, i32, u32, u32, u32, u32, C.POINTER(f32), C.POINTER(f32)]),
        "vr_volume_bytes": (C.c_uint64, [vp]),
        "vr_debug_read_volume": (i32, [vp, vp]),
        "vr_debug_read_volume_native": (i32, [vp, vp]),
        "vr_debug_volume_info": (i32, [vp, C.POINTER(u32), C.POINTER(f32), C.POINTER(i32)]),
        "vr_set_transfer_function": (i32, [vp, C.POINTER(u32), u32]),
        "vr_set_slicing": (i32, [vp, C.POINTER(f32), C.POINTER(f32)]),
        "vr_render": (i32, [vp, C.POINTER(vr_camera), C.POINTER(vr_params), vp, i32]),
        "vr_render_device": (i32, [vp, C.POINTER(vr_camera), C.POINTER(vr_params), vp, i32, u32, u32, u32, vp]),
        "vr_shard_rows": (u32, [u32, u32, u32]),
        "vr_assemble_rows": (i32, [vp, vp, vp, i32, u32, u32, vp]),
        "vr_count_work": (i32, [vp, C.POINTER(vr_camera), C.POINTER(vr_params), u32, u32, u32, C.POINTER(vr_stats)]),
        "vr_timing_enable": (i32, [vp, i32]),
        "vr_timing_read": (i32, [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
        "vr_timing_reset": (i32, [vp]),
        "vr_kernel_name": (C.c_char_p, [vp, C.POINTER(vr_params)]),
        "vr_import_memory_fd": (C.c_int, [vp, C.c_int, C.c_uint64, C.c_uint64, C.POINTER(vp),
                                          C.POINTER(vp)]),
        "vr_release_external_memory": (C.c_int, [vp, vp]),
        "vr_debug_set_knob": (i32, [vp, i32, i32]),
        "vr_debug_timing_member": (i32, [vp, i32, C.POINTER(vr_member_timing)]),
        "vr_debug_host_profile_enable": (i32, [vp, i32]),
        "vr_debug_host_profile_member": (i32, [vp, i32, C.POINTER(vr_dist_host_profile)]),
        "vr_set_row_share": (i32, [vp, u32, u32]),
        "vr_get_row_share": (i32, [vp, C.POINTER(u32), C.POINTER(u32)]),
        "vr_shard_rows_ctx": (u32, [vp, u32, u32, u32]),
        "vr_set_memory_budget": (i32, [vp, C.c_uint64]),
        "vr_memory_report": (i32, [vp, C.POINTER(vr_memory_info)]),
        "vr_prepare": (i32, [vp, C.POINTER(vr_camera), C.POINTER(vr_params)]),
        "vr_debug_get_knob": (i32, [vp, i32, C.POINTER(i32)]),
        "vr_set_render_mode": (i32, [vp, i32]),
        "vr_get_render_mode": (i32, [vp, C.POINTER(i32)]),
        "vr_set_isovalue": (i32, [vp, C.c_float]),
        "vr_get_isovalue": (i32, [vp, C.POINTER(C.c_float)]),
        "vr_mpr_render": (i32, [vp, C.POINTER(vr_mpr_plane), C.POINTER(vr_params), vp, i32]),
        "vr_mpr_render_device": (i32, [vp, C.POINTER(vr_mpr_plane), C.POINTER(vr_params), vp, i32, vp]),
        "vr_mpr_count_work": (i32, [vp, C.POINTER(vr_mpr_plane), C.POINTER(vr_params),
                                    C.POINTER(vr_stats)]),
        "vr_mpr_axis_plane": (i32, [i32, f32, u32, u32, u32, f32, i32, C.POINTER(vr_mpr_plane)]),
        "vr_histogram": (i32, [vp, C.POINTER(vr_hist_request), C.POINTER(C.c_uint64),
                               C.POINTER(vr_hist_info)]),
        "vr_hist_edges": (i32, [f32, f32, u32, C.POINTER(f32)]),
        "vr_hist_window": (i32, [C.POINTER(C.c_uint64), u32, f32, f32, C.c_double, C.c_double,
                                 C.POINTER(f32), C.POINTER(f32)]),
        "vr_set_value_range": (i32, [vp, f32, f32]),
        "vr_hit_render": (i32, [vp, C.POINTER(vr_camera), C.POINTER(vr_params),
                                C.POINTER(vr_hit_request), vp]),
        "vr_hit_render_device": (i32, [vp, C.POINTER(vr_camera), C.POINTER(vr_params),
                                       C.POINTER(vr_hit_request), vp, vp]),
        "vr_hit_count_work": (i32, [vp, C.POINTER(vr_camera), C.POINTER(vr_params),
                                    C.POINTER(vr_hit_request), C.POINTER(vr_stats)]),
        "vr_pick": (i32, [vp, C.POINTER(vr_camera), C.POINTER(vr_params), C.POINTER(vr_hit_request),
                          u32, u32, C.POINTER(vr_hit)]),
        "vr_mesh_write_ply": (i32, [C.c_char_p, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(f32),
                                    C.POINTER(f32)]),
        "vr_label_count": (i32, [vp, C.POINTER(vr_label_request), C.POINTER(vr_label_info)]),
        "vr_label_components": (i32, [vp, C.POINTER(vr_label_request), vp, C.c_uint64, vp, C.c_uint64,
                                      C.POINTER(vr_label_info)]),
        "vr_label_components_device": (i32, [vp, C.POINTER(vr_label_request), vp, C.c_uint64, vp,
                                             C.c_uint64, C.POINTER(vr_label_info), vp]),
        "vr_region_grow": (i32, [vp, C.POINTER(vr_label_request), C.POINTER(C.c_uint32), vp, C.c_uint64,
                                 C.POINTER(vr_label_component)]),
        "vr_region_grow_device": (i32, [vp, C.POINTER(vr_label_request), C.POINTER(C.c_uint32), vp,
                                        C.c_uint64, C.POINTER(vr_label_component), vp]),
        "vr_mesh_count": (i32, [vp, C.POINTER(vr_mesh_request), C.POINTER(vr_mesh_info)]),
        "vr_mesh_extract": (i32, [vp, C.POINTER(vr_mesh_request), vp, C.c_uint64, vp, C.c_uint64,
                                  C.POINTER(vr_mesh_info)]),
        "vr_mesh_extract_device": (i32, [vp, C.POINTER(vr_mesh_request), vp, C.c_uint64, vp, C.c_uint64,
                                         C.POINTER(vr_mesh_info), vp]),
        "vr_debug_create_members": (vp, [C.POINTER(i32), i32, u32, u32, i32]),
        "vr_debug_fail_member": (i32, [vp, i32, C.c_uint64]),
        "vr_debug_variant_name": (i32, [C.POINTER(vr_variant_facts), C.c_char_p, C.c_size_t]),
        "vr_debug_last_kernel_name": (C.c_char_p, [vp]),
        "vr_debug_label_pass_ms": (i32, [vp, C.POINTER(C.c_float)]),
        "vr_debug_ymajor_copy_bytes": (C.c_uint64, [vp]),
        "vr_debug_ymajor_field_bytes": (C.c_uint64, [vp]),
        "vr_cam_init": (None, [C.POINTER(vr_orbit_camera)]),
        "vr_cam_rotate": (None, [C.POINTER(vr_orbit_camera), f32, f32]),
        "vr_cam_zoom": (None, [C.POINTER(vr_orbit_camera), f32]),
        "vr_cam_position": (None, [C.POINTER(vr_orbit_camera), C.POINTER(f32)]),
        "vr_cam_view": (None, [C.POINTER(vr_orbit_camera), C.POINTER(f32)]),
        "vr_cam_to_camera": (None, [C.POINTER(vr_orbit_camera), C.POINTER(vr_camera)]),
        "vr_gradient_create": (vp, []),
        "vr_gradient_destroy": (None, [vp]),
        "vr_gradient_add_color_marker": (i32, [vp, f32, f32, f32, f32]),
        "vr_gradient_add_alpha_marker": (i32, [vp, f32, f32]),
        "vr_gradient_remove_color_marker": (i32, [vp, C.c_size_t]),
        "vr_gradient_remove_alpha_marker": (i32, [vp, C.c_size_t]),
        "vr_gradient_set_alpha_marker": (i32, [vp, C.c_size_t, f32, f32]),
        "vr_gradient_set_color_marker": (i32, [vp, C.c_size_t, f32, f32, f32, f32]),
        "vr_gradient_marker_count": (C.c_size_t, [vp, i32]),
        "vr_gradient_sample": (None, [vp, f32, C.POINTER(f32)]),
        "vr_gradient_discretize": (i32, [vp, C.c_size_t, C.POINTER(u32)]),
        "vr_nrrd_load": (i32, [C.c_char_p, C.POINTER(vr_dataset)]),
        "vr_nrrd_write_raw": (i32, [C.c_char_p, vp, i32, C.POINTER(u32)]),
        "vr_csv_load": (i32, [C.POINTER(C.c_char_p), C.c_size_t, C.POINTER(vr_dataset)]),
        "vr_dataset_free": (None, [C.POINTER(vr_dataset)]),
        "vr_host_last_error": (C.c_char_p, []),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    if L.vr_abi_version() != ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH} has ABI {L.vr_abi_version()}, this binding expects "
                           f"{ABI_VERSION}: rebuild it")
    _LIB = L
    return L


def _family_signatures() -> dict:
    """family -> {entry point: (restype, argtypes)} of the libraries beside libvr_amd.so."""
    vp, u32, u64, i32, f32, P = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_float, C.POINTER
    ext, name = P(u32), (C.c_char_p, [vp])
    ei, mi, li, si = P(vr_edt_info), P(vr_morph_info), P(vr_label_info), P(vr_mask_select_info)
    req, hr, hi = P(vr_mask_select_request), P(vr_hist_request), P(vr_hist_info)
    ti, reg = P(vr_mstat_info), P(vr_mstat_region)
    cam, par, src, pl = P(vr_camera), P(vr_params), P(vr_mview_source), P(vr_mpr_plane)
    vi, oi = P(vr_mview_info), P(vr_mview_occ_info)
    mq, mmi = P(vr_mmesh_request), P(vr_mmesh_info)
    return {
        "morph": {
            "vr_edt_squared_device": (i32, [vp, ext, vp, u32, u32, vp, u64, ei, vp]),
            "vr_edt_squared": (i32, [vp, ext, vp, u32, u32, vp, u64, ei]),
            "vr_mask_morph_device": (i32, [vp, ext, u32, u32, vp, u32, vp, u64, mi, vp]),
            "vr_mask_morph": (i32, [vp, ext, u32, u32, vp, u32, vp, u64, mi]),
            "vr_morph_last_kernel_name": name,
        },
        "maskcc": {
            "vr_mask_label_device": (i32, [vp, ext, vp, u32, u32, vp, u64, vp, u64, li, vp]),
            "vr_mask_label": (i32, [vp, ext, vp, u32, u32, vp, u64, vp, u64, li]),
            "vr_mask_select_device": (i32, [vp, ext, req, vp, u32, vp, u64, si, vp]),
            "vr_mask_select": (i32, [vp, ext, req, vp, u32, vp, u64, si]),
            "vr_maskcc_last_kernel_name": name,
            "vr_debug_maskcc_pass_ms": (i32, [vp, P(f32)]),  # (a debug hook, in no header)
        },
        "mstat": {
            "vr_mask_stats_device": (i32, [vp, ext, ext, vp, u32, hr, vp, hi, reg, vp]),
            "vr_mask_stats": (i32, [vp, ext, ext, vp, u32, hr, vp, hi, reg]),
            "vr_label_stats_device": (i32, [vp, ext, ext, vp, vp, u64, vp, u64, ti, vp]),
            "vr_label_stats": (i32, [vp, ext, ext, vp, vp, u64, vp, u64, ti]),
            "vr_mask_window_device": (i32, [vp, ext, ext, vp, u32, f32, f32, vp, u64, mi, vp]),
            "vr_mask_window": (i32, [vp, ext, ext, vp, u32, f32, f32, vp, u64, mi]),
            "vr_mstat_last_kernel_name": name,
        },
        "mview": {
            "vr_mview_occupancy_words": (u64, [ext]),
            "vr_mask_occupancy_device": (i32, [vp, src, vp, u64, oi, vp]),
            "vr_mask_hit_render_device": (i32, [vp, cam, par, src, ext, vp, u64, vi, vp]),
            "vr_mask_hit_render": (i32, [vp, cam, par, src, ext, vp, u64, vi]),
            "vr_mask_pick": (i32, [vp, cam, par, src, u32, u32, P(vr_mask_hit)]),
            "vr_mask_slice_device": (i32, [vp, pl, src, vp, u64, vi, vp]),
            "vr_mask_slice": (i32, [vp, pl, src, vp, u64, vi]),
            "vr_mview_last_kernel_name": name,
        },
        "mmesh": {
            "vr_mask_mesh_count_device": (i32, [vp, mq, mmi, vp]),
            "vr_mask_mesh_count": (i32, [vp, mq, mmi]),
            "vr_mask_mesh_extract_device": (i32, [vp, mq, vp, u64, vp, u64, mmi, vp]),
            "vr_mask_mesh_extract": (i32, [vp, mq, vp, u64, vp, u64, mmi]),
            "vr_mmesh_last_kernel_name": name,
        },
    }


# family -> (the environment variable that names its library, the file beside LIB_PATH otherwise)
FAMILY_LIBS = {"morph": ("VR_AMD_MORPH_LIB", "libvr_amd_morph.so"),
               "maskcc": ("VR_AMD_MASKCC_LIB", "libvr_amd_maskcc.so"),
               "mstat": ("VR_AMD_MSTAT_LIB", "libvr_amd_mstat.so"),
               "mview": ("VR_AMD_MVIEW_LIB", "libvr_amd_mview.so"),
               "mmesh": ("VR_AMD_MMESH_LIB", "libvr_amd_mmesh.so")}
FAMILY_LIB_PATHS = {f: os.environ.get(env) or os.path.join(os.path.dirname(LIB_PATH), so)
                    for f, (env, so) in FAMILY_LIBS.items()}
MORPH_LIB_PATH, MASKCC_LIB_PATH, MSTAT_LIB_PATH = (FAMILY_LIB_PATHS[f] for f in ("morph", "maskcc", "mstat"))
MVIEW_LIB_PATH = FAMILY_LIB_PATHS["mview"]
MMESH_LIB_PATH = FAMILY_LIB_PATHS["mmesh"]
_FAMILY_LIBS = {}


def family_lib(family: str) -> C.CDLL:
    """Load lib/libvr_amd_<family>.so (vr_<family>.h) on first use, after lib(): it takes the host
    scaffold from libvr_amd.so.  Fails loudly: there is no fallback path."""
    if family in _FAMILY_LIBS:
        return _FAMILY_LIBS[family]
    lib()
    path = FAMILY_LIB_PATHS[family]
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: build it with `make -C volumetric-renderer_amd` "
                           "(or __graft_entry__.build()); there is no CPU fallback")
    L = C.CDLL(path)
    for name, (res, args) in _family_signatures()[family].items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _FAMILY_LIBS[family] = L
    return L


def morph_lib() -> C.CDLL:
    return family_lib("morph")


def maskcc_lib() -> C.CDLL:
    return family_lib("maskcc")


def mstat_lib() -> C.CDLL:
    return family_lib("mstat")


def mview_lib() -> C.CDLL:
    return family_lib("mview")


def mmesh_lib() -> C.CDLL:
    return family_lib("mmesh")


def mmesh_request(ext, array_ptr: int, elem_bytes: int, origin=(0, 0, 0), label=None, closed=True, normals=True,
                  smooth_iters: int = 0, relax: float = 0.5, select=None, reserved: int = 0) -> vr_mmesh_request:
    """A vr_mmesh_request of the (bx, by, bz) = ext grid at `origin`: label None matches every non-zero
    element (MVIEW_ANY), a label that element alone (MVIEW_LABEL)."""
    q = vr_mmesh_request()
    for a in range(3):
        q.ext[a] = int(ext[a]) & 0xFFFFFFFF
        q.origin[a] = int(origin[a]) & 0xFFFFFFFF
    q.elem_bytes = int(elem_bytes) & 0xFFFFFFFF
    q.select = (MVIEW_ANY if label is None else MVIEW_LABEL) if select is None else int(select) & 0xFFFFFFFF
    q.label = 0 if label is None else int(label) & 0xFFFFFFFF
    q.closed = int(closed) & 0xFFFFFFFF
    q.normals = int(normals) & 0xFFFFFFFF
    q.smooth_iters = int(smooth_iters) & 0xFFFFFFFF
    q.relax = float(relax)
    q.reserved = int(reserved) & 0xFFFFFFFF
    q.array = array_ptr or None
    return q


def mview_source(ext, array_ptr: int, elem_bytes: int, origin=(0, 0, 0), label=None, occupancy_ptr: int = 0,
                 select=None, reserved: int = 0) -> vr_mview_source:
    """A vr_mview_source of the (bx, by, bz) = ext grid at `origin`: label None matches every non-zero
    element (MVIEW_ANY), a label that element alone (MVIEW_LABEL)."""
    s = vr_mview_source()
    for a in range(3):
        s.ext[a] = int(ext[a]) & 0xFFFFFFFF
        s.origin[a] = int(origin[a]) & 0xFFFFFFFF
    s.elem_bytes = int(elem_bytes) & 0xFFFFFFFF
    s.select = (MVIEW_ANY if label is None else MVIEW_LABEL) if select is None else int(select) & 0xFFFFFFFF
    s.label = 0 if label is None else int(label) & 0xFFFFFFFF
    s.reserved = int(reserved) & 0xFFFFFFFF
    s.array = array_ptr or None
    s.occupancy = occupancy_ptr or None
    return s


def mview_occupancy_words(ext) -> int:
    """vr_mview_occupancy_words of the (bx, by, bz) grid."""
    return int(mview_lib().vr_mview_occupancy_words((C.c_uint32 * 3)(*[int(v) & 0xFFFFFFFF for v in ext])))


def mstat_region_dict(r: vr_mstat_region) -> dict:
    return {"label": r.label, "voxels": r.voxels, "nan": r.nan, "vmin": r.vmin, "vmax": r.vmax,
            "min_index": r.min_index, "max_index": r.max_index, "sum": r.sum, "sum2": r.sum2}


def mask_select_request(rule: int, connectivity: int = 6, min_voxels: int = 0, seed=(0, 0, 0)) -> vr_mask_select_request:
    """A vr_mask_select_request; seed: the (i, j, k) grid voxel of MASK_KEEP_SEED."""
    req = vr_mask_select_request()
    req.rule = int(rule) & 0xFFFFFFFF
    req.connectivity = int(connectivity) & 0xFFFFFFFF
    req.min_voxels = int(min_voxels)
    req.seed[:] = [int(v) & 0xFFFFFFFF for v in seed]
    return req


def mpr_plane(origin, du, dv, dn, width: int, height: int, nsamples: int = 1,
              op: int = OP_MAX) -> vr_mpr_plane:
    """A vr_mpr_plane from texture-space vectors (rounded to f32 as the struct holds them)."""
    pl = vr_mpr_plane()
    for name, v in (("origin", origin), ("du", du), ("dv", dv), ("dn", dn)):
        for a in range(3):
            getattr(pl, name)[a] = float(v[a])
    pl.width, pl.height, pl.nsamples, pl.op = int(width), int(height), int(nsamples), int(op)
    return pl


def axis_plane(axis: int, position: float, width: int, height: int, nsamples: int = 1,
               spacing: float = 0.0, op: int = OP_MAX) -> vr_mpr_plane:
    """vr_mpr_axis_plane: the axis-aligned plane (AXIS_SAGITTAL / AXIS_CORONAL / AXIS_AXIAL) at
    `position` showing the whole cross-section; ValueError where the C function refuses."""
    pl = vr_mpr_plane()
    rc = lib().vr_mpr_axis_plane(int(axis), float(position), int(width), int(height), int(nsamples),
                                 float(spacing), int(op), C.byref(pl))
    if rc != 0:
        raise ValueError(f"vr_mpr_axis_plane failed ({rc}): {lib().vr_last_error(None).decode()}")
    return pl


def hit_request(kind: int, threshold: float = 0.5, rect=None) -> vr_hit_request:
    """A vr_hit_request: the kind, OPACITY's threshold, and the pixel rectangle (x0, y0, w, h) or
    None for the whole framebuffer."""
    req = vr_hit_request()
    req.kind, req.threshold = int(kind), float(threshold)
    if rect is not None:
        req.use_rect = 1
        for a in range(4):
            req.rect[a] = int(rect[a])
    return req


def mesh_request(iso: float, closed=True, normals=True, box=None) -> vr_mesh_request:
    """A vr_mesh_request: the isovalue (density units), the two flags, and the voxel box
    ((x0, y0, z0), (x1, y1, z1)), half open, or None for the whole volume."""
    req = vr_mesh_request()
    req.iso, req.closed, req.normals = float(iso), int(closed), int(normals)
    if box is not None:
        req.use_box = 1
        for a in range(3):
            req.box_min[a], req.box_max[a] = int(box[0][a]), int(box[1][a])
    return req


def label_request(lo: float, hi: float, connectivity=6, box=None) -> vr_label_request:
    """A vr_label_request: the window [lo, hi] (density units, either may be infinite), the
    connectivity (6 or 26) and the voxel box ((x0, y0, z0), (x1, y1, z1)), half open, or None for
    the whole volume."""
    req = vr_label_request()
    req.lo, req.hi, req.connectivity = float(lo), float(hi), int(connectivity)
    if box is not None:
        req.use_box = 1
        for a in range(3):
            req.box_min[a], req.box_max[a] = int(box[0][a]), int(box[1][a])
    return req


def label_component_dict(comp: vr_label_component) -> dict:
    return {"label": comp.label, "voxels": comp.voxels, "bbox_min": tuple(comp.bbox_min),
            "bbox_max": tuple(comp.bbox_max), "sum": tuple(comp.sum)}


def write_ply(path: str, verts, tris, scale=None, offset=None) -> None:
    """vr_mesh_write_ply: verts (MESH_VERTEX_DTYPE) and tris ((T, 3) uint32) as a binary PLY, the
    positions at pos * scale + offset."""
    v = np.ascontiguousarray(verts, MESH_VERTEX_DTYPE)
    t = np.ascontiguousarray(tris, np.uint32)
    sc = (C.c_float * 3)(*scale) if scale is not None else None
    of = (C.c_float * 3)(*offset) if offset is not None else None
    rc = lib().vr_mesh_write_ply(os.fsencode(path), v.ctypes.data if v.size else None, v.size,
                                 t.ctypes.data if t.size else None, t.size // 3, sc, of)
    if rc != 0:
        raise RuntimeError(f"vr_mesh_write_ply failed ({rc}): {lib().vr_host_last_error().decode()}")


def hist_edges(lo: float, hi: float, nbins: int) -> np.ndarray:
    """vr_hist_edges: the nbins lower bin edges (float32); ValueError where the C function refuses."""
    e = np.empty(max(int(nbins), 0) if 0 <= int(nbins) <= HIST_MAX_BINS else 0, np.float32)
    rc = lib().vr_hist_edges(float(lo), float(hi), int(nbins) & 0xFFFFFFFF,
                             e.ctypes.data_as(C.POINTER(C.c_float)))
    if rc != 0:
        raise ValueError(f"vr_hist_edges failed ({rc}): {lib().vr_last_error(None).decode()}")
    return e


def hist_window(bins, lo: float, hi: float, p_lo: float, p_hi: float):
    """vr_hist_window: (vmin, vmax) as float32 of the percentile window [p_lo, p_hi] of a histogram
    over [lo, hi]; ValueError where the C function refuses."""
    b = np.ascontiguousarray(bins, dtype=np.uint64)
    v0, v1 = C.c_float(), C.c_float()
    rc = lib().vr_hist_window(b.ctypes.data_as(C.POINTER(C.c_uint64)), b.size, float(lo), float(hi),
                              float(p_lo), float(p_hi), C.byref(v0), C.byref(v1))
    if rc != 0:
        raise ValueError(f"vr_hist_window failed ({rc}): {lib().vr_last_error(None).decode()}")
    return np.float32(v0.value), np.float32(v1.value)


def default_params(**overrides) -> vr_params:
    p = vr_params()
    lib().vr_params_default(C.byref(p))
    for k, v in overrides.items():
        if k == "clear_color":
            for i in range(4):
                p.clear_color[i] = v[i]
        else:
            setattr(p, k, v)
    return p


# --------------------------------------------------------------------------------------
# Inputs that feed the pass (C++ restatements in host/vr_host.cpp)
# --------------------------------------------------------------------------------------
class OrbitCamera:
    """Vol::Scene::Camera (src/scene/camera.cpp:7-48), via vr_cam_*."""

    def __init__(self):
        self._c = vr_orbit_camera()
        lib().vr_cam_init(C.byref(self._c))

    def rotate(self, dx: float, dy: float) -> "OrbitCamera":
        lib().vr_cam_rotate(C.byref(self._c), dx, dy)
        return self

    def zoom(self, delta: float) -> "OrbitCamera":
        lib().vr_cam_zoom(C.byref(self._c), delta)
        return self

    def set_radius(self, r: float) -> "OrbitCamera":
        self._c.radius = r
        return self

    @property
    def radius(self) -> float:
        return float(self._c.radius)

    def get_position(self) -> np.ndarray:
        out = (C.c_float * 3)()
        lib().vr_cam_position(C.byref(self._c), out)
        return np.array(out[:], dtype=np.float32)

    def get_view(self) -> np.ndarray:
        out = (C.c_float * 16)()
        lib().vr_cam_view(C.byref(self._c), out)
        return np.array(out[:], dtype=np.float32)

    def to_vr_camera(self) -> vr_camera:
        cam = vr_camera()
        lib().vr_cam_to_camera(C.byref(self._c), C.byref(cam))
        return cam


def make_camera(radius: float = 3.0, rotate=None) -> OrbitCamera:
    cam = OrbitCamera()
    if rotate is not None:
        cam.rotate(float(rotate[0]), float(rotate[1]))
    cam.set_radius(radius)
    return cam


class Gradient:
    """Vol::UI::Components::Gradient (src/ui/components/gradient.cpp), via vr_gradient_*."""

    def __init__(self):
        self._g = lib().vr_gradient_create()

    def __del__(self):
        if getattr(self, "_g", None):
            lib().vr_gradient_destroy(self._g)
            self._g = None

    def add_color_marker(self, loc, rgb) -> int:
        return lib().vr_gradient_add_color_marker(self._g, loc, *[float(x) for x in rgb])

    def add_alpha_marker(self, loc, a) -> int:
        return lib().vr_gradient_add_alpha_marker(self._g, loc, float(a))

    def remove_color_marker(self, i) -> bool:
        return bool(lib().vr_gradient_remove_color_marker(self._g, i))

    def remove_alpha_marker(self, i) -> bool:
        return bool(lib().vr_gradient_remove_alpha_marker(self._g, i))

    def set_alpha_marker(self, i, loc, a) -> int:
        return lib().vr_gradient_set_alpha_marker(self._g, i, loc, float(a))

    def set_color_marker(self, i, loc, rgb) -> int:
        return lib().vr_gradient_set_color_marker(self._g, i, loc, *[float(x) for x in rgb])

    def marker_count(self, alpha: bool) -> int:
        return int(lib().vr_gradient_marker_count(self._g, 1 if alpha else 0))

    def sample(self, loc) -> np.ndarray:
        out = (C.c_float * 4)()
        lib().vr_gradient_sample(self._g, loc, out)
        return np.array(out[:], dtype=np.float32)

    def discretize(self, count: int = 256) -> np.ndarray:
        out = (C.c_uint32 * count)()
        if lib().vr_gradient_discretize(self._g, count, out) != 0:
            raise RuntimeError("discretize failed")
        return np.array(out[:], dtype=np.uint32)


@dataclass
class Dataset:
    """Vol::Data::Dataset (src/data/dataset.h:9-13), kept in the file's native dtype."""
    dims: tuple
    vmin: float
    vmax: float
    data: np.ndarray  # shape (nz, ny, nx), native dtype, x fastest


def _take_dataset(ds: vr_dataset) -> Dataset:
    dims = tuple(int(x) for x in ds.dims)
    npdt = DTYPE_TO_NP[ds.dtype]
    n = dims[0] * dims[1] * dims[2]
    buf = (C.c_char * (n * npdt.itemsize)).from_address(ds.data)
    # one copy out of the library's buffer, which is freed below
    arr = np.frombuffer(buf, dtype=npdt).reshape(dims[2], dims[1], dims[0]).copy()
    out = Dataset(dims, float(ds.vmin), float(ds.vmax), arr)
    lib().vr_dataset_free(C.byref(ds))
    return out


def load_nrrd(path: str) -> Dataset:
    """NrrdFileParser::parse (nrrd_file_parser.cpp:21-47); raises RuntimeError like the reference."""
    ds = vr_dataset()
    rc = lib().vr_nrrd_load(path.encode(), C.byref(ds))
    if rc != 0:
        raise RuntimeError(lib().vr_host_last_error().decode())
    return _take_dataset(ds)


def load_csv(paths: Sequence[str]) -> Dataset:
    """CsvFileParser::parse (csv_file_parser.cpp:14-50)."""
    arr = (C.c_char_p * len(paths))(*[p.encode() for p in paths])
    ds = vr_dataset()
    rc = lib().vr_csv_load(arr, len(paths), C.byref(ds))
    if rc != 0:
        raise RuntimeError(lib().vr_host_last_error().decode())
    return _take_dataset(ds)


def write_nrrd_raw(nhdr_path: str, data: np.ndarray) -> None:
    """Write data (nz, ny, nx) as a detached raw NRRD pair (nhdr + raw)."""
    data = np.ascontiguousarray(data)
    dims = (C.c_uint32 * 3)(data.shape[2], data.shape[1], data.shape[0])
    rc = lib().vr_nrrd_write_raw(nhdr_path.encode(), data.ctypes.data, NP_TO_DTYPE[data.dtype], dims)
    if rc != 0:
        raise RuntimeError(lib().vr_host_last_error().decode())


# --------------------------------------------------------------------------------------
# The pass
# --------------------------------------------------------------------------------------
class OffscreenPass:
    """Mirror of Vol::Rendering::OffscreenPass (offscreen_pass.h:40-54) over the C ABI."""

    def __init__(self, width: int, height: int, device: int = 0, device_mask: Optional[int] = None,
                 members: Optional[Sequence[int]] = None, exchange: int = EXCHANGE_COPY):
        """device: the HIP device (vr_create); device_mask: render every frame across these
        devices instead (vr_create_mask, bit d = device d); members: an explicit member list
        whose devices may repeat (vr_debug_create_members, the one-GPU rehearsal), with the
        shards reaching member 0 by `exchange` (EXCHANGE_COPY or EXCHANGE_RCCL)."""
        L = lib()
        self.n_members = len(members) if members is not None else (
            1 if device_mask is None else bin(device_mask).count("1"))
        if members is not None:
            devs = (C.c_int * len(members))(*members)
            self._ctx = L.vr_debug_create_members(devs, len(members), width, height, exchange)
            what = "vr_debug_create_members"
        elif device_mask is None:
            self._ctx = L.vr_create(device, width, height)
            what = "vr_create"
        else:
            self._ctx = L.vr_create_mask(device_mask, width, height)
            what = "vr_create_mask"
        if not self._ctx:
            raise RuntimeError(f"{what} failed: {L.vr_last_error(None).decode()}")

    # -- lifecycle --
    def close(self):
        if getattr(self, "_ctx", None):
            lib().vr_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown: module globals may already be gone
            pass

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): {lib().vr_last_error(self._ctx).decode()}")

    @property
    def device_mask(self) -> int:
        m = C.c_uint32()
        self._check(lib().vr_get_device_mask(self._ctx, C.byref(m)), "vr_get_device_mask")
        return int(m.value)

    @property
    def size(self):
        w, h = C.c_uint32(), C.c_uint32()
        self._check(lib().vr_get_size(self._ctx, C.byref(w), C.byref(h)), "vr_get_size")
        return int(w.value), int(h.value)

    # -- reference setters --
    def framebuffer_size_changed(self, width: int, height: int):
        self._check(lib().vr_resize(self._ctx, width, height), "framebuffer_size_changed")

    def volume_dataset_changed(self, dataset: Dataset):
        data = np.ascontiguousarray(dataset.data)
        nx, ny, nz = dataset.dims
        assert data.size == nx * ny * nz, "dataset dims do not match data"
        self._check(lib().vr_set_volume(self._ctx, data.ctypes.data, NP_TO_DTYPE[data.dtype],
                                        nx, ny, nz, float(dataset.vmin), float(dataset.vmax)),
                    "volume_dataset_changed")

    def volume_dataset_changed_device(self, ptr: int, dtype, dims, vmin, vmax, stream: int = 0):
        nx, ny, nz = dims
        self._check(lib().vr_set_volume_device(self._ctx, C.c_void_p(ptr), NP_TO_DTYPE[np.dtype(dtype)],
                                               nx, ny, nz, float(vmin), float(vmax),
                                               C.c_void_p(stream or None)),
                    "volume_dataset_changed(device)")

    def generate_volume(self, dims, dtype=np.float32, seed: int = 2024, kind: int = 0):
        lo, hi = C.c_float(), C.c_float()
        self._check(lib().vr_generate_volume(self._ctx, kind, NP_TO_DTYPE[np.dtype(dtype)],
                                             dims[0], dims[1], dims[2], seed,
                                             C.byref(lo), C.byref(hi)), "vr_generate_volume")
        return float(lo.value), float(hi.value)

    def read_volume(self, native: bool = False) -> np.ndarray:
        """The resident volume as (nz, ny, nx) float32, or (native=True) in its storage type
        (uint8/int8/uint16/int16/float32: 1/4 of the host memory for 8-bit volumes)."""
        dims, mm, st = self.volume_info()
        shape = (dims[2], dims[1], dims[0])
        if native:
            out = np.empty(shape, dtype=(np.uint8, np.int8, np.uint16, np.int16, np.float32)[st])
            self._check(lib().vr_debug_read_volume_native(self._ctx, out.ctypes.data),
                        "vr_debug_read_volume_native")
            return out
        out = np.empty(shape, dtype=np.float32)
        self._check(lib().vr_debug_read_volume(self._ctx, out.ctypes.data), "vr_debug_read_volume")
        return out

    def volume_info(self):
        dims = (C.c_uint32 * 3)()
        mm = (C.c_float * 2)()
        st = C.c_int()
        self._check(lib().vr_debug_volume_info(self._ctx, dims, mm, C.byref(st)), "vr_debug_volume_info")
        return tuple(dims[:]), (float(mm[0]), float(mm[1])), int(st.value)

    def volume_bytes(self) -> int:
        return int(lib().vr_volume_bytes(self._ctx))

    def slicing_changed(self, vmin, vmax):
        a = (C.c_float * 3)(*[float(x) for x in vmin])
        b = (C.c_float * 3)(*[float(x) for x in vmax])
        self._check(lib().vr_set_slicing(self._ctx, a, b), "slicing_changed")

    def transfer_function_changed(self, data):
        arr = np.ascontiguousarray(np.asarray(data, dtype=np.uint32))
        ptr = arr.ctypes.data_as(C.POINTER(C.c_uint32))
        self._check(lib().vr_set_transfer_function(self._ctx, ptr, int(arr.size)),
                    "transfer_function_changed")

    def render_mode_changed(self, mode: int):
        """vr_set_render_mode (vr_modes.h): MODE_COMPOSITE, MODE_MIP, MODE_ISO, MODE_MINIP or
        MODE_MEAN for the frames that follow."""
        self._check(lib().vr_set_render_mode(self._ctx, int(mode)), "render_mode_changed")

    @property
    def render_mode(self) -> int:
        m = C.c_int()
        self._check(lib().vr_get_render_mode(self._ctx, C.byref(m)), "vr_get_render_mode")
        return int(m.value)

    def isovalue_changed(self, v: float):
        """vr_set_isovalue (vr_iso.h): the MODE_ISO surface's density, in the volume's units."""
        self._check(lib().vr_set_isovalue(self._ctx, C.c_float(v)), "isovalue_changed")

    @property
    def isovalue(self) -> float:
        v = C.c_float()
        self._check(lib().vr_get_isovalue(self._ctx, C.byref(v)), "vr_get_isovalue")
        return float(v.value)

    # -- record/render --
    def render(self, camera: OrbitCamera, params: Optional[vr_params] = None,
               out_format: int = OUT_RGBA32F, out: Optional[np.ndarray] = None) -> np.ndarray:
        """Synchronous full frame into host memory: (H, W, 4) float32 or uint8 (into `out`
        when given, e.g. a buffer reused frame after frame)."""
        w, h = self.size
        p = params if params is not None else default_params()
        cam = camera.to_vr_camera() if isinstance(camera, OrbitCamera) else camera
        dt = np.float32 if out_format == OUT_RGBA32F else np.uint8
        if out is None:
            out = np.empty((h, w, 4), dtype=dt)
        elif out.shape != (h, w, 4) or out.dtype != dt or not out.flags.c_contiguous:
            raise ValueError(f"out must be a C-contiguous ({h}, {w}, 4) {np.dtype(dt).name} array")
        self._check(lib().vr_render(self._ctx, C.byref(cam), C.byref(p), out.ctypes.data, out_format),
                    "render")
        return out

    # -- multi-planar reformat (vr_mpr.h): its own image size, no camera, no render mode --
    def render_mpr(self, plane: vr_mpr_plane, params: Optional[vr_params] = None,
                   out_format: int = OUT_RGBA32F) -> np.ndarray:
        """vr_mpr_render: the plane's (height, width, 4) image, float32 or uint8."""
        p = params if params is not None else default_params()
        out = np.empty((plane.height, plane.width, 4),
                       dtype=np.float32 if out_format == OUT_RGBA32F else np.uint8)
        self._check(lib().vr_mpr_render(self._ctx, C.byref(plane), C.byref(p), out.ctypes.data,
                                        out_format), "render_mpr")
        return out

    def render_mpr_device(self, plane: vr_mpr_plane, params: Optional[vr_params], out_ptr: int,
                          out_format: int = OUT_RGBA8, stream: int = 0):
        p = params if params is not None else default_params()
        self._check(lib().vr_mpr_render_device(self._ctx, C.byref(plane), C.byref(p),
                                               C.c_void_p(out_ptr), out_format,
                                               C.c_void_p(stream or None)), "render_mpr_device")

    # -- value histogram and value window (vr_hist.h) --
    def histogram(self, nbins: int, lo: Optional[float] = None, hi: Optional[float] = None,
                  box=None):
        """vr_histogram of the resident volume: (uint64 counts, info dict).  lo / hi default to
        the context's window; box = ((x0, y0, z0), (x1, y1, z1)), half open, in voxels."""
        if lo is None or hi is None:
            w = self.volume_info()[1]
            lo = w[0] if lo is None else lo
            hi = w[1] if hi is None else hi
        req = vr_hist_request()
        req.lo, req.hi, req.nbins = float(lo), float(hi), int(nbins)
        if box is not None:
            req.use_box = 1
            for a in range(3):
                req.box_min[a], req.box_max[a] = int(box[0][a]), int(box[1][a])
        bins = np.zeros(min(max(int(nbins), 1), HIST_MAX_BINS), np.uint64)
        info = vr_hist_info()
        self._check(lib().vr_histogram(self._ctx, C.byref(req),
                                       bins.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(info)),
                    "histogram")
        return bins, {"voxels": info.voxels, "below": info.below, "above": info.above,
                      "nan": info.nan, "vmin": np.float32(info.vmin), "vmax": np.float32(info.vmax)}

    def value_range_changed(self, vmin: float, vmax: float) -> None:
        """vr_set_value_range: a new value window for the resident voxels (no re-upload)."""
        self._check(lib().vr_set_value_range(self._ctx, float(vmin), float(vmax)),
                    "value_range_changed")

    # -- hit records and picking (vr_hit.h): where a pixel of the 3D frame comes from --
    def hit_image(self, camera, params, kind: int, threshold: float = 0.5, rect=None) -> np.ndarray:
        """vr_hit_render: the (h, w) HIT_DTYPE records of the framebuffer, or of the pixel
        rectangle rect = (x0, y0, w, h)."""
        cam = camera.to_vr_camera() if isinstance(camera, OrbitCamera) else camera
        p = params if params is not None else default_params()
        req = hit_request(kind, threshold, rect)
        w, h = (int(rect[2]), int(rect[3])) if rect is not None else self.size
        out = np.empty((max(h, 0), max(w, 0)), HIT_DTYPE)
        self._check(lib().vr_hit_render(self._ctx, C.byref(cam), C.byref(p), C.byref(req),
                                        out.ctypes.data if out.size else None), "hit_image")
        return out

    def hit_image_device(self, camera, params, kind: int, out_ptr: int, threshold: float = 0.5,
                         rect=None, stream: int = 0):
        cam = camera.to_vr_camera() if isinstance(camera, OrbitCamera) else camera
        p = params if params is not None else default_params()
        req = hit_request(kind, threshold, rect)
        self._check(lib().vr_hit_render_device(self._ctx, C.byref(cam), C.byref(p), C.byref(req),
                                               C.c_void_p(out_ptr), C.c_void_p(stream or None)),
                    "hit_image_device")

    def pick(self, camera, params, px: int, py: int, kind: int, threshold: float = 0.5) -> np.ndarray:
        """vr_pick: the HIT_DTYPE record (a 0-d array) of framebuffer pixel (px, py)."""
        cam = camera.to_vr_camera() if isinstance(camera, OrbitCamera) else camera
        p = params if params is not None else default_params()
        req = hit_request(kind, threshold, None)
        out = vr_hit()
        self._check(lib().vr_pick(self._ctx, C.byref(cam), C.byref(p), C.byref(req), int(px), int(py),
                                  C.byref(out)), "pick")
        return np.frombuffer(bytes(out), HIT_DTYPE)[0]

    def hit_count_work(self, camera, params, kind: int, threshold: float = 0.5, rect=None) -> dict:
        cam = camera.to_vr_camera() if isinstance(camera, OrbitCamera) else camera
        p = params if params is not None else default_params()
        req = hit_request(kind, threshold, rect)
        st = vr_stats()
        self._check(lib().vr_hit_count_work(self._ctx, C.byref(cam), C.byref(p), C.byref(req),
                                            C.byref(st)), "hit_count_work")
        return dict(rays=st.rays, samples=st.samples, shaded_samples=st.shaded_samples,
                    steps=st.steps, skipped_samples=st.skipped_samples)

    # -- the isosurface as a triangle mesh (vr_mesh.h) --
    def _mesh_request(self, iso, closed, normals, box) -> vr_mesh_request:
        return mesh_request(self.isovalue if iso is None else iso, closed, normals, box)

    @staticmethod
    def _mesh_info(info: vr_mesh_info) -> dict:
        return {"vertices": info.vertices, "triangles": info.triangles,
                "inside_voxels": info.inside_voxels}

    def mesh_count(self, iso: Optional[float] = None, closed=True, normals=True, box=None) -> dict:
        """vr_mesh_count: the vertices, triangles and inside voxels of the mesh at `iso` (default:
        the context's isovalue)."""
        req = self._mesh_request(iso, closed, normals, box)
        info = vr_mesh_info()
        self._check(lib().vr_mesh_count(self._ctx, C.byref(req), C.byref(info)), "mesh_count")
        return self._mesh_info(info)

    def mesh(self, iso: Optional[float] = None, closed=True, normals=True, box=None):
        """vr_mesh_extract: (vertices as MESH_VERTEX_DTYPE records, triangles (T, 3) uint32, info
        dict).  Sized by vr_mesh_count first."""
        req = self._mesh_request(iso, closed, normals, box)
        info = vr_mesh_info()
        self._check(lib().vr_mesh_count(self._ctx, C.byref(req), C.byref(info)), "mesh_count")
        nv, nt = int(info.vertices), int(info.triangles)
        verts = np.zeros(max(nv, 1), MESH_VERTEX_DTYPE)  # (never a NULL buffer)
        tris = np.zeros((max(nt, 1), 3), np.uint32)
        self._check(lib().vr_mesh_extract(self._ctx, C.byref(req), verts.ctypes.data, nv,
                                          tris.ctypes.data, nt, C.byref(info)), "mesh")
        return verts[:nv], tris[:nt], self._mesh_info(info)

    def mesh_device(self, verts_ptr: int, vcap: int, tris_ptr: int, tcap: int,
                    iso: Optional[float] = None, closed=True, normals=True, box=None,
                    stream: int = 0) -> dict:
        """vr_mesh_extract_device: the mesh into device memory (vcap vertex records, tcap
        triangles) on `stream`; returns the info dict when both buffers are complete."""
        req = self._mesh_request(iso, closed, normals, box)
        info = vr_mesh_info()
        self._check(lib().vr_mesh_extract_device(self._ctx, C.byref(req), C.c_void_p(verts_ptr), int(vcap),
                                                 C.c_void_p(tris_ptr), int(tcap), C.byref(info),
                                                 C.c_void_p(stream or None)), "mesh_device")
        return self._mesh_info(info)

    # -- connected components and region growing (vr_label.h) --
    LABEL_PASSES = ("local", "seam", "flatten", "scan", "table_init", "accumulate", "largest", "grow")

    def label_pass_ms(self) -> dict:
        """vr_debug_label_pass_ms: kernel ms of each pass of the last label or region-grow call
        (timing enabled), by name."""
        ms = (C.c_float * 8)()
        self._check(lib().vr_debug_label_pass_ms(self._ctx, ms), "label_pass_ms")
        return dict(zip(self.LABEL_PASSES, (float(v) for v in ms)))

    @staticmethod
    def _label_info(info: vr_label_info) -> dict:
        return {"voxels": info.voxels, "in_voxels": info.in_voxels, "components": info.components,
                "largest_voxels": info.largest_voxels, "largest_label": info.largest_label}

    def _label_shape(self, box):
        """(bz, by, bx) of the box, or of the volume.  (A box the library will refuse -- empty or
        inverted -- gives empty axes here: the call is still made, and raises.)"""
        if box is not None:
            return tuple(max(int(box[1][a]) - int(box[0][a]), 0) for a in (2, 1, 0))
        d = self.volume_info()[0]
        return (int(d[2]), int(d[1]), int(d[0]))

    def label_count(self, lo: float, hi: float, connectivity=6, box=None) -> dict:
        """vr_label_count: the voxels, in voxels, components and largest component of the window."""
        req = label_request(lo, hi, connectivity, box)
        info = vr_label_info()
        self._check(lib().vr_label_count(self._ctx, C.byref(req), C.byref(info)), "label_count")
        return self._label_info(info)

    def label(self, lo: float, hi: float, connectivity=6, box=None):
        """vr_label_components: (labels (bz, by, bx) uint32, records as LABEL_COMPONENT_DTYPE sorted
        by label, info dict).  One labelling where the table has at most 65536 records; a larger
        one is sized by the first call's VR_ENOSPC info and labelled once more."""
        req = label_request(lo, hi, connectivity, box)
        info = vr_label_info()
        shape = self._label_shape(box)
        n = shape[0] * shape[1] * shape[2]
        labels = np.zeros(max(n, 1), np.uint32)  # (never a NULL buffer)
        cap = 1 << 16
        comps = np.zeros(cap, LABEL_COMPONENT_DTYPE)
        rc = lib().vr_label_components(self._ctx, C.byref(req), labels.ctypes.data, n,
                                       comps.ctypes.data, cap, C.byref(info))
        if rc == ENOSPC and int(info.voxels) == n and int(info.components) > cap:
            cap = int(info.components)
            comps = np.zeros(cap, LABEL_COMPONENT_DTYPE)
            rc = lib().vr_label_components(self._ctx, C.byref(req), labels.ctypes.data, n,
                                           comps.ctypes.data, cap, C.byref(info))
        self._check(rc, "label")
        return labels[:n].reshape(shape), comps[:int(info.components)], self._label_info(info)

    def label_device(self, labels_ptr: int, lcap: int, comps_ptr: int, ccap: int, lo: float, hi: float,
                     connectivity=6, box=None, stream: int = 0) -> dict:
        """vr_label_components_device: lcap labels and ccap records into device memory on `stream`;
        returns the info dict when both buffers are complete."""
        req = label_request(lo, hi, connectivity, box)
        info = vr_label_info()
        self._check(lib().vr_label_components_device(self._ctx, C.byref(req), C.c_void_p(labels_ptr), int(lcap),
                                                     C.c_void_p(comps_ptr), int(ccap), C.byref(info),
                                                     C.c_void_p(stream or None)), "label_device")
        return self._label_info(info)

    def region_grow(self, seed, lo: float, hi: float, connectivity=6, box=None):
        """vr_region_grow: (mask (bz, by, bx) uint8 of the seed's component, its record as a dict).
        seed: the (x, y, z) volume voxel index."""
        req = label_request(lo, hi, connectivity, box)
        shape = self._label_shape(box)
        n = shape[0] * shape[1] * shape[2]
        mask = np.zeros(max(n, 1), np.uint8)  # (never a NULL buffer)
        comp = vr_label_component()
        sd = (C.c_uint32 * 3)(*[int(v) & 0xFFFFFFFF for v in seed])
        self._check(lib().vr_region_grow(self._ctx, C.byref(req), sd, mask.ctypes.data, n,
                                         C.byref(comp)), "region_grow")
        return mask[:n].reshape(shape), label_component_dict(comp)

    def region_grow_device(self, seed, mask_ptr: int, mcap: int, lo: float, hi: float, connectivity=6,
                           box=None, stream: int = 0) -> dict:
        """vr_region_grow_device: the mask into device memory (mcap bytes) on `stream`; returns the
        component's record when the mask is complete."""
        req = label_request(lo, hi, connectivity, box)
        comp = vr_label_component()
        sd = (C.c_uint32 * 3)(*[int(v) for v in seed])
        self._check(lib().vr_region_grow_device(self._ctx, C.byref(req), sd, C.c_void_p(mask_ptr), int(mcap),
                                                C.byref(comp), C.c_void_p(stream or None)), "region_grow_device")
        return label_component_dict(comp)

    # -- distance transform and ball morphology (vr_morph.h, lib/libvr_amd_morph.so) --
    @staticmethod
    def _edt_info(info: vr_edt_info) -> dict:
        return {"voxels": info.voxels, "target_voxels": info.target_voxels, "max_dist2": info.max_dist2,
                "max_index": info.max_index}

    @staticmethod
    def _morph_info(info: vr_morph_info) -> dict:
        return {"voxels": info.voxels, "in_set": info.in_set, "out_set": info.out_set}

    @staticmethod
    def _morph_mask(mask):
        """A (bz, by, bx) uint8 or uint32 array -> (the contiguous array, ext, elem_bytes)."""
        m = np.ascontiguousarray(mask)
        if m.ndim != 3 or m.dtype not in (np.dtype(np.uint8), np.dtype(np.uint32)):
            raise ValueError("a mask is a (bz, by, bx) array of uint8 or uint32")
        return m, (C.c_uint32 * 3)(m.shape[2], m.shape[1], m.shape[0]), m.dtype.itemsize

    def distance_transform(self, mask, to_set=True) -> dict:
        """vr_edt_squared: {"dist2": (bz, by, bx) uint32, "info": dict} -- the exact squared distance
        of every voxel to the nearest set voxel of `mask` (to_set) or the nearest unset one."""
        m, ext, eb = self._morph_mask(mask)
        out = np.zeros(max(m.size, 1), np.uint32)  # (never a NULL buffer)
        info = vr_edt_info()
        self._check(morph_lib().vr_edt_squared(self._ctx, ext, m.ctypes.data, eb,
                                               EDT_TO_SET if to_set else EDT_TO_UNSET, out.ctypes.data, m.size,
                                               C.byref(info)), "distance_transform")
        return {"dist2": out[:m.size].reshape(m.shape), "info": self._edt_info(info)}

    def distance_transform_device(self, ext, mask_ptr: int, elem_bytes: int, dist2_ptr: int, dcap: int,
                                  to_set=True, stream: int = 0) -> dict:
        """vr_edt_squared_device: dcap distances into device memory on `stream`; returns the info
        dict when the buffer is complete.  ext: (bx, by, bz)."""
        info = vr_edt_info()
        self._check(morph_lib().vr_edt_squared_device(
            self._ctx, self._u3(ext), C.c_void_p(mask_ptr), int(elem_bytes),
            EDT_TO_SET if to_set else EDT_TO_UNSET, C.c_void_p(dist2_ptr), int(dcap), C.byref(info),
            C.c_void_p(stream or None)), "distance_transform_device")
        return self._edt_info(info)

    def morph(self, mask, op: int, r2: int) -> dict:
        """vr_mask_morph: {"mask": (bz, by, bx) uint8 of 0/1, "info": dict} -- MORPH_DILATE, _ERODE,
        _OPEN or _CLOSE of `mask` with the ball of squared radius r2."""
        m, ext, eb = self._morph_mask(mask)
        out = np.zeros(max(m.size, 1), np.uint8)  # (never a NULL buffer)
        info = vr_morph_info()
        self._check(morph_lib().vr_mask_morph(self._ctx, ext, int(op), int(r2), m.ctypes.data, eb,
                                              out.ctypes.data, m.size, C.byref(info)), "morph")
        return {"mask": out[:m.size].reshape(m.shape), "info": self._morph_info(info)}

    def morph_device(self, ext, op: int, r2: int, mask_ptr: int, elem_bytes: int, out_ptr: int, mcap: int,
                     stream: int = 0) -> dict:
        """vr_mask_morph_device: mcap mask bytes into device memory on `stream`; returns the info
        dict when the buffer is complete.  ext: (bx, by, bz)."""
        info = vr_morph_info()
        self._check(morph_lib().vr_mask_morph_device(
            self._ctx, self._u3(ext), int(op), int(r2), C.c_void_p(mask_ptr),
            int(elem_bytes), C.c_void_p(out_ptr), int(mcap), C.byref(info), C.c_void_p(stream or None)),
            "morph_device")
        return self._morph_info(info)

    def morph_last_kernel_name(self) -> str:
        return morph_lib().vr_morph_last_kernel_name(self._ctx).decode()

    # -- the components of a mask: labels, selection, hole filling (vr_maskcc.h, lib/libvr_amd_maskcc.so) --
    @staticmethod
    def _select_info(info: vr_mask_select_info) -> dict:
        return {"voxels": info.voxels, "in_set": info.in_set, "out_set": info.out_set,
                "components": info.components, "kept": info.kept}

    def mask_label(self, mask, connectivity=6):
        """vr_mask_label: (labels (bz, by, bx) uint32, records as LABEL_COMPONENT_DTYPE sorted by
        label, info dict) of a (bz, by, bx) uint8 or uint32 mask.  One labelling where the table has
        at most 65536 records; a larger one is sized by the first call's VR_ENOSPC info and labelled
        once more."""
        m, ext, eb = self._morph_mask(mask)
        info = vr_label_info()
        labels = np.zeros(max(m.size, 1), np.uint32)  # (never a NULL buffer)
        cap = 1 << 16
        comps = np.zeros(cap, LABEL_COMPONENT_DTYPE)
        call = lambda: maskcc_lib().vr_mask_label(self._ctx, ext, m.ctypes.data, eb, int(connectivity),
                                                  labels.ctypes.data, m.size, comps.ctypes.data, cap, C.byref(info))
        rc = call()
        if rc == ENOSPC and int(info.voxels) == m.size and int(info.components) > cap:
            cap = int(info.components)
            comps = np.zeros(cap, LABEL_COMPONENT_DTYPE)
            rc = call()
        self._check(rc, "mask_label")
        return labels[:m.size].reshape(m.shape), comps[:int(info.components)], self._label_info(info)

    def mask_label_device(self, ext, mask_ptr: int, elem_bytes: int, labels_ptr: int, lcap: int, comps_ptr: int,
                          ccap: int, connectivity=6, stream: int = 0) -> dict:
        """vr_mask_label_device: lcap labels and ccap records into device memory on `stream`; returns
        the info dict when both buffers are complete.  ext: (bx, by, bz)."""
        info = vr_label_info()
        self._check(maskcc_lib().vr_mask_label_device(
            self._ctx, self._u3(ext), C.c_void_p(mask_ptr), int(elem_bytes),
            int(connectivity), C.c_void_p(labels_ptr), int(lcap), C.c_void_p(comps_ptr), int(ccap), C.byref(info),
            C.c_void_p(stream or None)), "mask_label_device")
        return self._label_info(info)

    def mask_select(self, mask, rule: int, connectivity=6, min_voxels: int = 0, seed=(0, 0, 0)) -> dict:
        """vr_mask_select: {"mask": (bz, by, bx) uint8 of 0/1, "info": dict} -- MASK_KEEP_LARGEST,
        _KEEP_MIN_VOXELS, _KEEP_SEED (seed: the (i, j, k) grid voxel) or MASK_FILL_HOLES."""
        m, ext, eb = self._morph_mask(mask)
        req = mask_select_request(rule, connectivity, min_voxels, seed)
        out = np.zeros(max(m.size, 1), np.uint8)  # (never a NULL buffer)
        info = vr_mask_select_info()
        self._check(maskcc_lib().vr_mask_select(self._ctx, ext, C.byref(req), m.ctypes.data, eb, out.ctypes.data,
                                                m.size, C.byref(info)), "mask_select")
        return {"mask": out[:m.size].reshape(m.shape), "info": self._select_info(info)}

    def mask_select_device(self, ext, rule: int, mask_ptr: int, elem_bytes: int, out_ptr: int, mcap: int,
                           connectivity=6, min_voxels: int = 0, seed=(0, 0, 0), stream: int = 0) -> dict:
        """vr_mask_select_device: mcap mask bytes into device memory on `stream`; returns the info
        dict when the buffer is complete.  ext: (bx, by, bz)."""
        req = mask_select_request(rule, connectivity, min_voxels, seed)
        info = vr_mask_select_info()
        self._check(maskcc_lib().vr_mask_select_device(
            self._ctx, self._u3(ext), C.byref(req), C.c_void_p(mask_ptr),
            int(elem_bytes), C.c_void_p(out_ptr), int(mcap), C.byref(info), C.c_void_p(stream or None)),
            "mask_select_device")
        return self._select_info(info)

    MASKCC_PASSES = ("rows", "link", "flatten", "scan", "table_init", "accumulate", "largest", "keep", "select")

    def maskcc_pass_ms(self) -> dict:
        """Kernel ms of each pass of the last mask_label* or mask_select* call (timing enabled), by name."""
        ms = (C.c_float * 9)()
        self._check(maskcc_lib().vr_debug_maskcc_pass_ms(self._ctx, ms), "maskcc_pass_ms")
        return dict(zip(self.MASKCC_PASSES, (float(v) for v in ms)))

    def maskcc_last_kernel_name(self) -> str:
        return maskcc_lib().vr_maskcc_last_kernel_name(self._ctx).decode()

    # -- the volume under a mask or a label array (vr_mstat.h, lib/libvr_amd_mstat.so) --
    @staticmethod
    def _u3(v):
        return (C.c_uint32 * 3)(*[int(x) & 0xFFFFFFFF for x in v])

    @staticmethod
    def _mstat_hist(hist):
        """hist = (nbins, lo, hi) or None -> (request or None, bins or None, info or None)."""
        if hist is None:
            return None, None, None
        req = vr_hist_request()
        req.nbins, req.lo, req.hi = int(hist[0]), float(hist[1]), float(hist[2])
        return req, np.zeros(min(max(int(hist[0]), 1), HIST_MAX_BINS), np.uint64), vr_hist_info()

    @staticmethod
    def _mstat_stats_result(region, bins, hinfo) -> dict:
        out = {"region": mstat_region_dict(region)}
        if bins is not None:
            out["bins"] = bins
            out["hist_info"] = {"voxels": hinfo.voxels, "below": hinfo.below, "above": hinfo.above,
                                "nan": hinfo.nan, "vmin": np.float32(hinfo.vmin), "vmax": np.float32(hinfo.vmax)}
        return out

    @staticmethod
    def _mstat_info(info: vr_mstat_info) -> dict:
        return {"voxels": info.voxels, "set": info.set, "unlisted": info.unlisted, "regions": info.regions}

    def mask_stats(self, mask, origin=(0, 0, 0), hist=None) -> dict:
        """vr_mask_stats: {"region": dict, and with hist = (nbins, lo, hi) "bins": uint64 counts,
        "hist_info": dict} of the volume under a (bz, by, bx) uint8 or uint32 mask whose voxel
        (0, 0, 0) is the volume voxel origin = (x, y, z)."""
        m, ext, eb = self._morph_mask(mask)
        req, bins, hinfo = self._mstat_hist(hist)
        region = vr_mstat_region()
        self._check(mstat_lib().vr_mask_stats(
            self._ctx, ext, self._u3(origin), m.ctypes.data, eb, C.byref(req) if req is not None else None,
            bins.ctypes.data if bins is not None else None, C.byref(hinfo) if hinfo is not None else None,
            C.byref(region)), "mask_stats")
        return self._mstat_stats_result(region, bins, hinfo)

    def mask_stats_device(self, ext, mask_ptr: int, elem_bytes: int, origin=(0, 0, 0), hist=None,
                          stream: int = 0) -> dict:
        """vr_mask_stats_device: the same of a mask in device memory, on `stream`.  ext: (bx, by, bz)."""
        req, bins, hinfo = self._mstat_hist(hist)
        region = vr_mstat_region()
        self._check(mstat_lib().vr_mask_stats_device(
            self._ctx, self._u3(ext), self._u3(origin), C.c_void_p(mask_ptr), int(elem_bytes),
            C.byref(req) if req is not None else None, bins.ctypes.data if bins is not None else None,
            C.byref(hinfo) if hinfo is not None else None, C.byref(region), C.c_void_p(stream or None)),
            "mask_stats_device")
        return self._mstat_stats_result(region, bins, hinfo)

    def label_stats(self, labels, table, origin=(0, 0, 0)):
        """vr_label_stats: (records as MSTAT_REGION_DTYPE in table order, info dict) of a (bz, by, bx)
        uint32 label array and a table of LABEL_COMPONENT_DTYPE records (only "label" is read)."""
        lab = np.ascontiguousarray(labels)
        if lab.ndim != 3 or lab.dtype != np.dtype(np.uint32):
            raise ValueError("a label array is a (bz, by, bx) array of uint32")
        tab = np.ascontiguousarray(table, LABEL_COMPONENT_DTYPE)
        n = int(tab.size)
        tab_buf = tab if n else np.zeros(1, LABEL_COMPONENT_DTYPE)  # (never a NULL buffer)
        out = np.zeros(max(n, 1), MSTAT_REGION_DTYPE)
        info = vr_mstat_info()
        self._check(mstat_lib().vr_label_stats(
            self._ctx, self._u3(lab.shape[::-1]), self._u3(origin), lab.ctypes.data, tab_buf.ctypes.data, n,
            out.ctypes.data, n, C.byref(info)), "label_stats")
        return out[:n], self._mstat_info(info)

    def label_stats_device(self, ext, labels_ptr: int, table_ptr: int, ntable: int, regions_ptr: int, rcap: int,
                           origin=(0, 0, 0), stream: int = 0) -> dict:
        """vr_label_stats_device: ntable records into device memory (rcap records) on `stream`; returns
        the info dict when they are complete.  ext: (bx, by, bz)."""
        info = vr_mstat_info()
        self._check(mstat_lib().vr_label_stats_device(
            self._ctx, self._u3(ext), self._u3(origin), C.c_void_p(labels_ptr), C.c_void_p(table_ptr), int(ntable),
            C.c_void_p(regions_ptr), int(rcap), C.byref(info), C.c_void_p(stream or None)), "label_stats_device")
        return self._mstat_info(info)

    def mask_window(self, mask, lo: float, hi: float, origin=(0, 0, 0), shape=None) -> dict:
        """vr_mask_window: {"mask": (bz, by, bx) uint8 of 0/1, "info": dict} -- the voxels of `mask`
        (None: of the whole (bz, by, bx) = shape grid) with lo <= f <= hi."""
        if mask is None:
            m, eb = None, 1
            shp = tuple(int(v) for v in shape)
            ext = self._u3(shp[::-1])
        else:
            m, ext, eb = self._morph_mask(mask)
            shp = m.shape
        n = shp[0] * shp[1] * shp[2]
        out = np.zeros(max(n, 1), np.uint8)  # (never a NULL buffer)
        info = vr_morph_info()
        self._check(mstat_lib().vr_mask_window(
            self._ctx, ext, self._u3(origin), m.ctypes.data if m is not None else None, eb, float(lo), float(hi),
            out.ctypes.data, n, C.byref(info)), "mask_window")
        return {"mask": out[:n].reshape(shp), "info": self._morph_info(info)}

    def mask_window_device(self, ext, mask_ptr: int, elem_bytes: int, lo: float, hi: float, out_ptr: int, mcap: int,
                           origin=(0, 0, 0), stream: int = 0) -> dict:
        """vr_mask_window_device: mcap mask bytes into device memory on `stream` (mask_ptr 0: every
        grid voxel is set); returns the info dict when the buffer is complete.  ext: (bx, by, bz)."""
        info = vr_morph_info()
        self._check(mstat_lib().vr_mask_window_device(
            self._ctx, self._u3(ext), self._u3(origin), C.c_void_p(mask_ptr or None), int(elem_bytes), float(lo),
            float(hi), C.c_void_p(out_ptr), int(mcap), C.byref(info), C.c_void_p(stream or None)),
            "mask_window_device")
        return self._morph_info(info)

    def mstat_last_kernel_name(self) -> str:
        return mstat_lib().vr_mstat_last_kernel_name(self._ctx).decode()

    # -- the view of a mask or a label array (vr_mview.h, lib/libvr_amd_mview.so) --
    @staticmethod
    def _mview_info(info: vr_mview_info) -> dict:
        return {n: int(getattr(info, n)) for n in ("voxels", "pixels", "covered", "hits", "steps", "samples")}

    @staticmethod
    def _rect(rect):
        return None if rect is None else (C.c_uint32 * 4)(*[int(v) & 0xFFFFFFFF for v in rect])

    def _mview_shape(self, rect):
        w, h = self.size
        return (h, w) if rect is None else (int(rect[3]), int(rect[2]))

    def mask_occupancy_device(self, source: vr_mview_source, occ_ptr: int, ocap_words: int, stream: int = 0) -> dict:
        """vr_mask_occupancy_device: the occupancy words of `source` into device memory (ocap_words
        words) on `stream`; returns the info dict when they are complete."""
        info = vr_mview_occ_info()
        self._check(mview_lib().vr_mask_occupancy_device(
            self._ctx, C.byref(source), C.c_void_p(occ_ptr), int(ocap_words), C.byref(info),
            C.c_void_p(stream or None)), "mask_occupancy_device")
        return {n: int(getattr(info, n)) for n in ("voxels", "cells", "cells_set", "matching")}

    def mask_hit_render(self, camera, params, array, origin=(0, 0, 0), label=None, rect=None):
        """vr_mask_hit_render: ((h, w) records as MVIEW_HIT_DTYPE, info dict) of a (bz, by, bx) uint8 or
        uint32 host array whose voxel (0, 0, 0) is the volume voxel origin = (x, y, z)."""
        m, ext, eb = self._morph_mask(array)
        cam = camera.to_vr_camera() if isinstance(camera, OrbitCamera) else camera
        src = mview_source(ext, m.ctypes.data, eb, origin, label)
        h, w = self._mview_shape(rect)
        out = np.zeros(max(h * w, 1), MVIEW_HIT_DTYPE)
        info = vr_mview_info()
        self._check(mview_lib().vr_mask_hit_render(
            self._ctx, C.byref(cam), C.byref(params), C.byref(src), self._rect(rect), out.ctypes.data, h * w,
            C.byref(info)), "mask_hit_render")
        return out[:h * w].reshape(h, w), self._mview_info(info)

    def mask_hit_render_device(self, camera, params, source: vr_mview_source, out_ptr: int, rcap: int, rect=None,
                               stream: int = 0) -> dict:
        """vr_mask_hit_render_device: the rectangle's records into device memory (rcap records) on
        `stream`; returns the info dict when they are complete."""
        cam = camera.to_vr_camera() if isinstance(camera, OrbitCamera) else camera
        info = vr_mview_info()
        self._check(mview_lib().vr_mask_hit_render_device(
            self._ctx, C.byref(cam), C.byref(params), C.byref(source), self._rect(rect), C.c_void_p(out_ptr),
            int(rcap), C.byref(info), C.c_void_p(stream or None)), "mask_hit_render_device")
        return self._mview_info(info)

    def mask_pick(self, camera, params, source: vr_mview_source, px: int, py: int) -> np.ndarray:
        """vr_mask_pick: the MVIEW_HIT_DTYPE record of framebuffer pixel (px, py) of a device array."""
        cam = camera.to_vr_camera() if isinstance(camera, OrbitCamera) else camera
        out = np.zeros(1, MVIEW_HIT_DTYPE)
        self._check(mview_lib().vr_mask_pick(
            self._ctx, C.byref(cam), C.byref(params), C.byref(source), int(px), int(py),
            C.cast(out.ctypes.data, C.POINTER(vr_mask_hit))), "mask_pick")
        return out[0]

    def mask_slice(self, plane: vr_mpr_plane, array, origin=(0, 0, 0), label=None):
        """vr_mask_slice: ((height, width) uint32 elements, info dict) of a host array on `plane`."""
        m, ext, eb = self._morph_mask(array)
        src = mview_source(ext, m.ctypes.data, eb, origin, label)
        n = int(plane.width) * int(plane.height)
        out = np.zeros(max(n, 1), np.uint32)
        info = vr_mview_info()
        self._check(mview_lib().vr_mask_slice(self._ctx, C.byref(plane), C.byref(src), out.ctypes.data, n,
                                              C.byref(info)), "mask_slice")
        return out[:n].reshape(int(plane.height), int(plane.width)), self._mview_info(info)

    def mask_slice_device(self, plane: vr_mpr_plane, source: vr_mview_source, out_ptr: int, pcap: int,
                          stream: int = 0) -> dict:
        """vr_mask_slice_device: the plane's elements into device memory (pcap uint32) on `stream`;
        returns the info dict when they are complete."""
        info = vr_mview_info()
        self._check(mview_lib().vr_mask_slice_device(
            self._ctx, C.byref(plane), C.byref(source), C.c_void_p(out_ptr), int(pcap), C.byref(info),
            C.c_void_p(stream or None)), "mask_slice_device")
        return self._mview_info(info)

    def mview_last_kernel_name(self) -> str:
        return mview_lib().vr_mview_last_kernel_name(self._ctx).decode()

    # -- the surface of a mask or of one label as a mesh (vr_mmesh.h, lib/libvr_amd_mmesh.so) --
    @staticmethod
    def _mmesh_info(info: vr_mmesh_info) -> dict:
        return {n: int(getattr(info, n)) for n in ("voxels", "vertices", "triangles", "matching")}

    def mask_mesh_count(self, array, origin=(0, 0, 0), label=None, closed=True) -> dict:
        """vr_mask_mesh_count: the info dict of a (bz, by, bx) uint8 or uint32 host array whose voxel
        (0, 0, 0) is the volume voxel origin = (x, y, z)."""
        m, ext, eb = self._morph_mask(array)
        req = mmesh_request(ext, m.ctypes.data, eb, origin, label, closed)
        info = vr_mmesh_info()
        self._check(mmesh_lib().vr_mask_mesh_count(self._ctx, C.byref(req), C.byref(info)), "mask_mesh_count")
        return self._mmesh_info(info)

    def mask_mesh_count_device(self, request: vr_mmesh_request, stream: int = 0) -> dict:
        """vr_mask_mesh_count_device: the info dict of a device array, known when it returns."""
        info = vr_mmesh_info()
        self._check(mmesh_lib().vr_mask_mesh_count_device(self._ctx, C.byref(request), C.byref(info),
                                                          C.c_void_p(stream or None)), "mask_mesh_count_device")
        return self._mmesh_info(info)

    def mask_mesh_extract(self, array, origin=(0, 0, 0), label=None, closed=True, normals=True, smooth_iters: int = 0,
                          relax: float = 0.5):
        """vr_mask_mesh_extract: (vertices as MESH_VERTEX_DTYPE records, triangles (T, 3) uint32, info
        dict) of a host array.  Sized by vr_mask_mesh_count first."""
        m, ext, eb = self._morph_mask(array)
        req = mmesh_request(ext, m.ctypes.data, eb, origin, label, closed, normals, smooth_iters, relax)
        info = vr_mmesh_info()
        self._check(mmesh_lib().vr_mask_mesh_count(self._ctx, C.byref(req), C.byref(info)), "mask_mesh_count")
        nv, nt = int(info.vertices), int(info.triangles)
        verts = np.zeros(max(nv, 1), MESH_VERTEX_DTYPE)  # (never a NULL buffer)
        tris = np.zeros((max(nt, 1), 3), np.uint32)
        self._check(mmesh_lib().vr_mask_mesh_extract(self._ctx, C.byref(req), verts.ctypes.data, nv, tris.ctypes.data,
                                                     nt, C.byref(info)), "mask_mesh_extract")
        return verts[:nv], tris[:nt], self._mmesh_info(info)

    def mask_mesh_extract_device(self, request: vr_mmesh_request, verts_ptr: int, vcap: int, tris_ptr: int, tcap: int,
                                 stream: int = 0) -> dict:
        """vr_mask_mesh_extract_device: the mesh of a device array into device memory (vcap vertex
        records, tcap triangles) on `stream`; returns the info dict when both buffers are complete."""
        info = vr_mmesh_info()
        self._check(mmesh_lib().vr_mask_mesh_extract_device(
            self._ctx, C.byref(request), C.c_void_p(verts_ptr), int(vcap), C.c_void_p(tris_ptr), int(tcap),
            C.byref(info), C.c_void_p(stream or None)), "mask_mesh_extract_device")
        return self._mmesh_info(info)

    def mmesh_last_kernel_name(self) -> str:
        return mmesh_lib().vr_mmesh_last_kernel_name(self._ctx).decode()

    def count_work_mpr(self, plane: vr_mpr_plane, params: Optional[vr_params] = None) -> dict:
        p = params if params is not None else default_params()
        st = vr_stats()
        self._check(lib().vr_mpr_count_work(self._ctx, C.byref(plane), C.byref(p), C.byref(st)),
                    "count_work_mpr")
        return dict(rays=st.rays, samples=st.samples, shaded_samples=st.shaded_samples,
                    steps=st.steps, skipped_samples=st.skipped_samples)

    def render_device(self, camera, params, out_ptr: int, out_format: int = OUT_RGBA8,
                      row_block: int = 16, rank: int = 0, nranks: int = 1, stream: int = 0):
        cam = camera.to_vr_camera() if isinstance(camera, OrbitCamera) else camera
        self._check(lib().vr_render_device(self._ctx, C.byref(cam), C.byref(params),
                                           C.c_void_p(out_ptr), out_format, row_block, rank,
                                           nranks, C.c_void_p(stream or None)), "render_device")

    def assemble_rows(self, gathered_ptr: int, out_ptr: int, out_format: int, row_block: int,
                      nranks: int, stream: int = 0):
        self._check(lib().vr_assemble_rows(self._ctx, C.c_void_p(gathered_ptr), C.c_void_p(out_ptr),
                                           out_format, row_block, nranks, C.c_void_p(stream or None)),
                    "assemble_rows")

    def count_work(self, camera, params, row_block=16, rank=0, nranks=1) -> dict:
        cam = camera.to_vr_camera() if isinstance(camera, OrbitCamera) else camera
        st = vr_stats()
        self._check(lib().vr_count_work(self._ctx, C.byref(cam), C.byref(params), row_block, rank,
                                        nranks, C.byref(st)), "count_work")
        return dict(rays=st.rays, samples=st.samples, shaded_samples=st.shaded_samples,
                    steps=st.steps, skipped_samples=st.skipped_samples)

    def timing_enable(self, on: bool = True):
        self._check(lib().vr_timing_enable(self._ctx, 1 if on else 0), "timing_enable")

    def timing_read(self):
        ms, n = C.c_double(), C.c_uint64()
        self._check(lib().vr_timing_read(self._ctx, C.byref(ms), C.byref(n)), "timing_read")
        return float(ms.value), int(n.value)

    def timing_reset(self):
        self._check(lib().vr_timing_reset(self._ctx), "timing_reset")

    def kernel_name(self, params) -> str:
        return lib().vr_kernel_name(self._ctx, C.byref(params)).decode()

    def last_kernel_name(self) -> str:
        """vr_debug_last_kernel_name: the kernel the last frame or count launch actually ran."""
        return lib().vr_debug_last_kernel_name(self._ctx).decode()

    def timing_member(self, member: int) -> dict:
        """vr_debug_timing_member: one device's summed kernel / render / gather / assembly ms."""
        t = vr_member_timing()
        self._check(lib().vr_debug_timing_member(self._ctx, member, C.byref(t)), "timing_member")
        return dict(device=int(t.device), frames=int(t.frames), kernel_ms=float(t.kernel_ms),
                    render_ms=float(t.render_ms), gather_ms=float(t.gather_ms),
                    assemble_ms=float(t.assemble_ms))

    # -- ABI 7: row shares, derived-structure memory, preparation --
    def fail_member(self, member: int, frame: int):
        """vr_debug_fail_member: member's enqueue of pipeline frame `frame` fails (VR_EIO)."""
        self._check(lib().vr_debug_fail_member(self._ctx, member, frame), "vr_debug_fail_member")

    def set_row_share(self, first_weight: int, other_weight: int):
        self._check(lib().vr_set_row_share(self._ctx, first_weight, other_weight), "set_row_share")

    def row_share(self):
        a, b = C.c_uint32(), C.c_uint32()
        self._check(lib().vr_get_row_share(self._ctx, C.byref(a), C.byref(b)), "row_share")
        return int(a.value), int(b.value)

    def shard_rows(self, height: int, row_block: int, nranks: int) -> int:
        return int(lib().vr_shard_rows_ctx(self._ctx, height, row_block, nranks))

    def set_memory_budget(self, nbytes: int):
        self._check(lib().vr_set_memory_budget(self._ctx, C.c_uint64(nbytes)), "set_memory_budget")

    def memory_report(self) -> dict:
        m = vr_memory_info()
        self._check(lib().vr_memory_report(self._ctx, C.byref(m)), "memory_report")
        r = {n: int(getattr(m, n)) for n, _ in vr_memory_info._fields_}
        # the y-major copy has no field of its own in the ABI 9 struct (vr_debug.h)
        r["ymajor_copy_bytes"] = int(lib().vr_debug_ymajor_copy_bytes(self._ctx))
        r["ymajor_field_bytes"] = int(lib().vr_debug_ymajor_field_bytes(self._ctx))
        return r

    def prepare(self, camera, params):
        cam = camera.to_vr_camera() if isinstance(camera, OrbitCamera) else camera
        self._check(lib().vr_prepare(self._ctx, C.byref(cam), C.byref(params)), "prepare")

    # -- include/vr/vr_debug.h: launch-policy overrides for tests (speed only, never results) --
    def host_profile_enable(self, on: bool = True):
        """vr_debug_host_profile_enable (multi-device contexts): per-member host enqueue time."""
        self._check(lib().vr_debug_host_profile_enable(self._ctx, int(bool(on))), "host_profile_enable")

    def host_profile_member(self, member: int) -> dict:
        """vr_debug_host_profile_member: member's host microseconds per frame, by step."""
        h = vr_dist_host_profile()
        self._check(lib().vr_debug_host_profile_member(self._ctx, member, C.byref(h)),
                    "host_profile_member")
        n = max(int(h.frames), 1)
        return dict(frames=int(h.frames), **{k: getattr(h, k) / n for k, _ in vr_dist_host_profile._fields_[1:]})

    def set_knob(self, name: str, value: int):
        self._check(lib().vr_debug_set_knob(self._ctx, KNOBS[name], int(value)), f"set_knob({name})")

    def get_knob(self, name: str) -> int:
        v = C.c_int()
        self._check(lib().vr_debug_get_knob(self._ctx, KNOBS[name], C.byref(v)), f"get_knob({name})")
        return int(v.value)

    @contextlib.contextmanager
    def knobs(self, **kw):
        """Set knobs for the duration of a with-block (auto values restored after)."""
        for k, v in kw.items():
            self.set_knob(k, v)
        try:
            yield self
        finally:
            for k in kw:
                self.set_knob(k, KNOB_AUTO[k])


def dist_unique_id() -> bytes:
    """Rank 0: a fresh RCCL communicator id (vr_dist_unique_id) to send to every rank."""
    buf = C.create_string_buffer(DIST_ID_BYTES)
    rc = lib().vr_dist_unique_id(buf)
    if rc:
        raise RuntimeError(f"vr_dist_unique_id failed ({rc}): {lib().vr_dist_last_error(None).decode()}")
    return buf.raw


class DistFrames:
    """Multi-GPU frames of one OffscreenPass over RCCL (include/vr/vr_dist.h): this rank's
    row blocks -> ncclGather to rank 0 -> de-interleave there, all stream-ordered, with
    `frames_in_flight` frames in flight.  Every rank constructs it together (it blocks until
    all `nranks` have joined) with the same communicator id."""

    def __init__(self, rp: "OffscreenPass", uid: bytes, nranks: int, rank: int,
                 row_block: int = 8, frames_in_flight: int = 3):
        if len(uid) != DIST_ID_BYTES:
            raise ValueError("communicator id must be DIST_ID_BYTES bytes")
        self.rank, self.nranks = rank, nranks
        self._rp = rp  # keeps the context alive
        self._d = lib().vr_dist_create(rp._ctx, C.create_string_buffer(uid, DIST_ID_BYTES),
                                       nranks, rank, row_block, frames_in_flight)
        if not self._d:
            raise RuntimeError(f"vr_dist_create failed: {lib().vr_dist_last_error(None).decode()}")

    def _check(self, rc: int, what: str):
        if rc:
            raise RuntimeError(f"{what} failed ({rc}): {lib().vr_dist_last_error(self._d).decode()}")

    def render(self, camera, params, frame_ptr: int = 0, stream: int = 0):
        """Enqueue one frame; rank 0's RGBA8 frame (H x W x 4 bytes at frame_ptr) is complete
        once `stream` passes this point."""
        cam = camera.to_vr_camera() if isinstance(camera, OrbitCamera) else camera
        self._check(lib().vr_dist_render(self._d, C.byref(cam), C.byref(params),
                                         C.c_void_p(frame_ptr or None), C.c_void_p(stream or None)),
                    "vr_dist_render")

    def synchronize(self):
        self._check(lib().vr_dist_synchronize(self._d), "vr_dist_synchronize")

    def timing_enable(self, on: bool = True):
        self._check(lib().vr_dist_timing_enable(self._d, 1 if on else 0), "vr_dist_timing_enable")

    def host_profile(self, enable=None):
        """Host microseconds per frame of each step vr_dist_render enqueues (vr_dist.h host
        profile), averaged since the last read, and the frames counted; enable=True/False
        switches the profiling first (then returns None)."""
        if enable is not None:
            self._check(lib().vr_dist_host_profile_enable(self._d, 1 if enable else 0),
                        "vr_dist_host_profile_enable")
            return None
        h = vr_dist_host_profile()
        self._check(lib().vr_dist_host_profile_read(self._d, C.byref(h)), "vr_dist_host_profile_read")
        n = max(int(h.frames), 1)
        return dict(frames=int(h.frames), **{k: getattr(h, k) / n for k, _ in vr_dist_host_profile._fields_[1:]})

    def timing_read(self):
        """(render ms, gather ms, frames) summed over the frames since timing was enabled (or
        last read): HIP events around this rank's render and its ncclGather."""
        r, g, n = C.c_double(), C.c_double(), C.c_uint64()
        self._check(lib().vr_dist_timing_read(self._d, C.byref(r), C.byref(g), C.byref(n)),
                    "vr_dist_timing_read")
        return r.value, g.value, n.value

    def close(self):
        if getattr(self, "_d", None):
            lib().vr_dist_destroy(self._d)
            self._d = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


KERNEL_SOURCES = ("csrc/vr_kernels.hip", "csrc/vr_internal.h", "csrc/vr_exact_math.h", "Makefile")


def kernel_source_hash() -> str:
    """sha256 (16 hex digits) of the kernel sources (round 4's key; kept for the record)."""
    import hashlib
    h = hashlib.sha256()
    for rel in KERNEL_SOURCES:
        with open(os.path.join(HERE, rel), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def _elf_sections(b: bytes, base: int = 0):
    import struct
    shoff = struct.unpack_from("<Q", b, base + 0x28)[0]
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", b, base + 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", b, base + shoff + i * shentsize) for i in range(shnum)]
    names = base + secs[shstrndx][4]
    return [(b[names + s[0]:b.index(b"\0", names + s[0])],) + s for s in secs]


def code_object_symbols(path: Optional[str] = None):
    """(name, bytes) of every sized symbol of the library's gfx950 code object (the
    `.hip_fatbin` ELF section): kernels' code bytes, and under `<kernel>.kd` their descriptors
    (register counts, LDS, kernarg size) with the layout-dependent code-entry offset zeroed."""
    import re
    import struct
    b = open(path or LIB_PATH, "rb").read()
    fb = [s for s in _elf_sections(b) if s[0] == b".hip_fatbin"]
    if not fb:
        raise RuntimeError(f"{path or LIB_PATH} has no .hip_fatbin section")
    fat = b[fb[0][5]:fb[0][5] + fb[0][6]]
    for p in (m.start() for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", fat)):
        q = p + 32
        for _ in range(struct.unpack_from("<Q", fat, p + 24)[0]):
            off, size, tl = struct.unpack_from("<QQQ", fat, q)
            triple = fat[q + 24:q + 24 + tl]
            q += 24 + tl
            if b"gfx950" not in triple:
                continue
            co = fat[p + off:p + off + size]
            secs = _elf_sections(co)
            st = next(s for s in secs if s[0] == b".symtab")
            strt = next(s for s in secs if s[0] == b".strtab")
            for i in range(st[6] // 24):
                nm, _, _, shndx, val, sz = struct.unpack_from("<IBBHQQ", co, st[5] + i * 24)
                name = co[strt[5] + nm:co.index(b"\0", strt[5] + nm)]
                if 0 < shndx < len(secs) and sz > 0:
                    sec = secs[shndx]
                    code = bytearray(co[sec[5] + val - sec[4]:sec[5] + val - sec[4] + sz])
                    if name.endswith(b".kd") and len(code) >= 24:
                        code[16:24] = bytes(8)  # kernel_code_entry_byte_offset
                    yield name, bytes(code)


def kernel_code_hash(path: Optional[str] = None) -> str:
    """sha256 (16 hex digits) of the frame kernels' machine code in the library: every
    instantiation of march_kernel, march_y_kernel (the y-major copy: the headline's view),
    march_pair_kernel (lane groups: small row shares) and order_tiles_kernel (the adaptive tile
    order inside a frame) -- gfx950 code bytes and kernel descriptor (code_object_symbols).
    Keys measured per-kernel figures (the PMC traffic bench.py's roofline reads) to the machine
    code they were measured on: host-only edits and changes to other kernels leave it
    unchanged, any change to a kernel a frame launches moves it (the build is deterministic;
    ADVICE r5: the pair and tile-order kernels were not hashed before)."""
    import hashlib
    syms = [(name, code) for name, code in code_object_symbols(path)
            if any(k in name for k in (b"12march_kernel", b"14march_y_kernel",
                                       b"17march_pair_kernel", b"18order_tiles_kernel"))]
    if not syms:
        raise RuntimeError(f"{path or LIB_PATH}: no march_kernel code in the gfx950 code object")
    h = hashlib.sha256()
    for name, code in sorted(syms):
        h.update(name)
        h.update(code)
    return h.hexdigest()[:16]


def variant_name(**facts) -> Optional[str]:
    """vr_debug_variant_name: the kernel a launch with these vr_variant_facts runs (None: none)."""
    buf = C.create_string_buffer(256)
    f = vr_variant_facts(**facts)
    return buf.value.decode() if lib().vr_debug_variant_name(C.byref(f), buf, len(buf)) == 0 else None


def shard_rows(height: int, row_block: int, nranks: int) -> int:
    return int(lib().vr_shard_rows(height, row_block, nranks))


def unorm8(img: np.ndarray) -> np.ndarray:
    """Float RGBA -> R8G8B8A8_UNORM exactly as the kernel stores it: (u8)(clamp*255 + 0.5)."""
    v = np.clip(np.nan_to_num(img.astype(np.float32), nan=0.0), np.float32(0), np.float32(1))
    return np.floor(v * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)
