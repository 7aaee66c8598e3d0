"""ctypes binding of libmvs_hip.so (include/mvs.h) for tests/ and bench.py.

Harness only: the product is the C-ABI library; its real host side is the C++ mirror of recon.hpp in
mesh-reconstruction_amd/host/.  This module fails loudly when the HIP library is missing -- there is
no CPU fallback (the oracle lives in oracle/ and is never imported from here).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.normpath(os.path.join(_HERE, "..", ".."))
# MVS_BUILD_VARIANT=san: the address / undefined-behaviour sanitized host build (`make sanitize`: san/lib, san/bin) instead of lib / bin
_VARIANT = os.environ.get("MVS_BUILD_VARIANT", "")
LIB_DIR = os.path.join(PKG_ROOT, _VARIANT, "lib") if _VARIANT else os.path.join(PKG_ROOT, "lib")
BIN_DIR = os.path.join(PKG_ROOT, _VARIANT, "bin") if _VARIANT else os.path.join(PKG_ROOT, "bin")
LIB_PATH = os.path.join(LIB_DIR, "libmvs_hip.so")

MVS_SWEEP_VOLUME = 1
MVS_SWEEP_FUSED_ARGMIN = 2
MVS_SWEEP_FORCE_GENERIC = 4
MVS_SWEEP_NO_RECT = 8
MVS_COST_ABSDIFF, MVS_COST_ZNCC = 0, 1
MVS_KEEP_ALL = 0
MVS_AGGREGATE_REFINE = 1
MVS_CLEAN_SCORES_AGGREGATED = 1
MVS_WINDOW_SELECT, MVS_WINDOW_REFINE = 1, 2
MVS_VOLUME_RAW, MVS_VOLUME_WINDOWED = 0, 1
MVS_FILTER_MEDIAN, MVS_FILTER_MEAN, MVS_FILTER_FILL = 1, 2, 4
MVS_PROPAGATE_SLOPES = 1
VOLUME_SOURCES = {"raw": MVS_VOLUME_RAW, "windowed": MVS_VOLUME_WINDOWED}
MVS_SHARD_ROWS, MVS_SHARD_VIEWS, MVS_SHARD_VIEWS_SCATTER = 0, 1, 2
SHARD_MODES = {"rows": 0, "views": 1, "views_scatter": 2}
MVS_SAMPLER_FIXED, MVS_SAMPLER_EXACT_F32 = 0, 1
SAMPLERS = {"fixed": MVS_SAMPLER_FIXED, "exact": MVS_SAMPLER_EXACT_F32}
MVS_K_SWEEP, MVS_K_ARGMIN, MVS_K_PLAN, MVS_K_RASTER, MVS_K_PROJECT, MVS_K_FLOW, MVS_K_FUSE, MVS_K_TSDF = 0, 1, 2, 3, 4, 5, 6, 7
MVS_K_COUNT = 8
BACKGROUND_DEPTH = np.float32(1.0)

# every symbol include/mvs.h declares: (name, restype, argtypes)
_vp, _i, _f, _sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
_fp, _u8p, _i32p, _u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
ABI = [
    ("mvs_create", _vp, [_i, _i, _i]),
    ("mvs_destroy", None, [_vp]),
    ("mvs_last_error", C.c_char_p, [_vp]),
    ("mvs_set_stream", _i, [_vp, _vp]),
    ("mvs_synchronize", _i, [_vp]),
    ("mvs_host_alloc", _vp, [_sz]),
    ("mvs_host_free", None, [_vp]),
    ("mvs_width", _i, [_vp]),
    ("mvs_height", _i, [_vp]),
    ("mvs_load_mesh", _i, [_vp, _fp, _i, _i32p, _i]),
    ("mvs_depth", _i, [_vp, _fp, _fp]),
    ("mvs_depth_probe", _i, [_vp, _fp, _i, _i32p, _i32p, _fp]),
    ("mvs_projected", _i, [_vp, _fp, _u8p, _fp, _u8p]),
    ("mvs_mix_background", _i, [_vp, _u8p, _u8p, _fp, _u8p]),
    ("mvs_compare", _i, [_vp, _u8p, _u8p, _fp]),
    ("mvs_flow_remap", _i, [_vp, _fp, _i, _u8p, _u8p]),
    ("mvs_flow", _i, [_vp, _u8p, _u8p, _i, _fp]),
    ("mvs_triangulate", _i, [_vp, _i, C.POINTER(_fp), _fp, _fp, _fp, _fp, C.POINTER(_i)]),
    ("mvs_process_frame", _i, [_vp, _fp, _u8p, _i, _fp, C.POINTER(_u8p), _i, _fp, C.POINTER(_i), _fp]),
    ("mvs_process_frame_slots", _i, [_vp, _fp, _i, _i, _fp, _i32p, _i, _fp, C.POINTER(_i), _fp]),
    ("mvs_filter_points", _i, [_vp, _fp, _i, _f, _i32p, C.POINTER(_i)]),
    ("mvs_filter_density_fetch", _i, [_vp, _fp]),
    ("mvs_filter_density_count", _i, [_vp]),
    ("mvs_sweep", _i, [_vp, _fp, _u8p, _i, _fp, C.POINTER(_u8p), _i, _f, _f, _fp, _fp, _fp]),
    ("mvs_warp_by_depth", _i, [_vp, _fp, _fp, _fp, _u8p, _u8p]),
    ("mvs_sweep_set_sampler", _i, [_vp, _i]),
    ("mvs_sweep_sampler", _i, [_vp]),
    ("mvs_sweep_set_main", _i, [_vp, _fp, _u8p]),
    ("mvs_sweep_set_views", _i, [_vp, _i, _fp, C.POINTER(_u8p)]),
    ("mvs_sweep_set_planes", _i, [_vp, _i, _f, _f]),
    ("mvs_sweep_set_main_device", _i, [_vp, _fp, _vp]),
    ("mvs_sweep_set_views_device", _i, [_vp, _i, _fp, C.POINTER(_vp)]),
    ("mvs_sweep_run", _i, [_vp, _i, _i, C.c_uint]),
    ("mvs_sweep_run_planes", _i, [_vp, _i, _i, _i, _i, C.c_uint]),
    ("mvs_sweep_plane_granularity", _i, []),
    ("mvs_sweep_run_rows", _i, [_vp, _i, _i, _i, _i, C.c_uint]),
    ("mvs_sweep_row_granularity", _i, []),
    ("mvs_sweep_row_granularity_of", _i, [_vp]),
    ("mvs_sweep_plan_shape", _i, [_vp]),
    ("mvs_resize_u8", _i, [_vp, _vp, _i, _i, _i, _vp, _i, _i]),
    ("mvs_set_texture_filter", _i, [_vp, _i]),
    ("mvs_texture_filter", _i, [_vp]),
    ("mvs_frame_store", _i, [_vp, _i]),
    ("mvs_frame_upload", _i, [_vp, _i, _vp]),
    ("mvs_frame_upload_device", _i, [_vp, _i, _vp]),
    ("mvs_set_lens", _i, [_vp, _fp, _f, _f]),
    ("mvs_lens", _i, [_vp, _fp, _fp, _fp]),
    ("mvs_undistort", _i, [_vp, _u8p, _u8p]),
    ("mvs_undistort_device", _i, [_vp, _vp, _vp, _i]),
    ("mvs_undistort_map", _i, [_vp, _fp]),
    ("mvs_frame_upload_lens", _i, [_vp, _i, _vp]),
    ("mvs_frame_upload_lens_device", _i, [_vp, _i, _vp]),
    ("mvs_sweep_handles", _i, [_vp, _i, _fp, _i, _vp, _vp, _i, _f, _f, _vp, _vp]),
    ("mvs_sweep_batch", _i, [_vp, _i, _vp, _vp, _i, _vp, _vp, _i, C.c_float, C.c_float, _vp, _vp]),
    ("mvs_sweep_batch_async", _i, [_vp, _i, _vp, _vp, _i, _vp, _vp, _i, C.c_float, C.c_float, _vp, _vp]),
    ("mvs_sweep_batch_wait", _i, [_vp]),
    ("mvs_depth_store", _i, [_vp, _i]),
    ("mvs_depth_upload", _i, [_vp, _i, _fp, _fp, _fp]),
    ("mvs_depth_upload_device", _i, [_vp, _i, _fp, _vp, _vp]),
    ("mvs_fuse_depth", _i, [_vp, _i, _i, _i32p, _i, _f, _f, _f, _fp, C.POINTER(_i)]),
    ("mvs_fuse_points_device", _vp, [_vp]),
    ("mvs_depth_support_upload", _i, [_vp, _i, _u8p]),
    ("mvs_depth_support_upload_device", _i, [_vp, _i, _vp]),
    ("mvs_depth_support_fetch", _i, [_vp, _i, _u8p]),
    ("mvs_depth_support_drop", _i, [_vp, _i]),
    ("mvs_fuse_depth_masked", _i, [_vp, _i, _i, _i32p, _i, _f, _f, _f, _i, _fp, C.POINTER(_i)]),
    ("mvs_propagate_normals", _i, [_vp, _fp]),
    ("mvs_propagate_normals_device", _vp, [_vp]),
    ("mvs_propagate_normals_fetch", _i, [_vp, _fp]),
    ("mvs_depth_normals_upload", _i, [_vp, _i, _fp]),
    ("mvs_depth_normals_upload_device", _i, [_vp, _i, _vp]),
    ("mvs_depth_normals_fetch", _i, [_vp, _i, _fp]),
    ("mvs_depth_normals_drop", _i, [_vp, _i]),
    ("mvs_fuse_depth_normals", _i, [_vp, _i, _i, _i32p, _i, _f, _f, _f, _i, _f, _fp, C.POINTER(_i)]),
    ("mvs_tsdf_integrate_masked", _i, [_vp, _i, _i32p, _i32p, _f, _i]),
    ("mvs_fuse_sequence", _i, [_vp, _i, _i32p, _i, _i32p, _i, _f, _f, _f, _i, C.c_longlong, _fp, _i32p, C.POINTER(C.c_longlong)]),
    ("mvs_fuse_sequence_points_device", _vp, [_vp]),
    ("mvs_depth_slot_matrices", _i, [_vp, _i, _fp]),
    ("mvs_tsdf_volume", _i, [_vp, _i, _fp, _f, _f]),
    ("mvs_tsdf_integrate", _i, [_vp, _i, _i32p, _f]),
    ("mvs_tsdf_fetch", _i, [_vp, _fp, _i32p]),
    ("mvs_tsdf_surface", _i, [_vp, _i, _vp]),
    ("mvs_tsdf_upload", _i, [_vp, _fp, _i32p]),
    ("mvs_tsdf_raycast", _i, [_vp, _fp, _i, _f]),
    ("mvs_tsdf_raycast_depth_device", _vp, [_vp]),
    ("mvs_tsdf_raycast_normals_device", _vp, [_vp]),
    ("mvs_tsdf_raycast_fetch", _i, [_vp, _fp, _fp]),
    ("mvs_tsdf_integrate_frames", _i, [_vp, _i, _i32p, _i32p, _f]),
    ("mvs_tsdf_appearance_fetch", _i, [_vp, _u32p]),
    ("mvs_tsdf_appearance_upload", _i, [_vp, _u32p]),
    ("mvs_tsdf_shade", _i, [_vp, _fp, _vp]),
    ("mvs_tsdf_shade_device", _vp, [_vp]),
    ("mvs_tsdf_shade_fetch", _i, [_vp, _u8p]),
    ("mvs_tsdf_sample_appearance", _i, [_vp, _fp, _i, _fp]),
    ("mvs_depth_slot_device", _vp, [_vp, _i]),
    ("mvs_sweep_argmin", _i, [_vp]),
    ("mvs_sweep_refine_depth", _i, [_vp]),
    ("mvs_sweep_aggregate", _i, [_vp, _i, _i, _i, _i, C.c_uint]),
    ("mvs_sweep_aggregated_device", _vp, [_vp, C.POINTER(_sz)]),
    ("mvs_sweep_aggregate_fetch", _i, [_vp, C.POINTER(C.c_uint16)]),
    ("mvs_sweep_clean", _i, [_vp, _i, _i, _i, _i, C.c_uint]),
    ("mvs_sweep_clean_report", _i, [_vp, C.POINTER(_i)]),
    ("mvs_sweep_clean_sizes_device", _vp, [_vp]),
    ("mvs_sweep_clean_sizes_fetch", _i, [_vp, _i32p]),
    ("mvs_sweep_window", _i, [_vp, _i, _i, _vp, C.c_uint]),
    ("mvs_sweep_windowed_device", _vp, [_vp, C.POINTER(_sz)]),
    ("mvs_sweep_window_fetch", _i, [_vp, _u32p]),
    ("mvs_sweep_set_volume_source", _i, [_vp, _i]),
    ("mvs_sweep_volume_source", _i, [_vp]),
    ("mvs_sweep_run_band", _i, [_vp, _i, _i, _vp, C.c_uint]),
    ("mvs_sweep_band_resolve", _i, [_vp]),
    ("mvs_sweep_band_depth_device", _vp, [_vp]),
    ("mvs_sweep_band_prior_device", _vp, [_vp]),
    ("mvs_sweep_band_fetch", _i, [_vp, _fp]),
    ("mvs_sweep_band_report", _i, [_vp, C.POINTER(_i)]),
    ("mvs_sweep_run_zncc", _i, [_vp, _i, _i, _i, C.c_uint]),
    ("mvs_sweep_run_bestk", _i, [_vp, _i, _i, _i, _i, _i, C.c_uint]),
    ("mvs_sweep_run_band_bestk", _i, [_vp, _i, _i, _vp, _i, _i, _i, C.c_uint]),
    ("mvs_sweep_run_bestk_gated", _i, [_vp, _i, _i, _i, _i, _i, _i, _vp, C.c_uint]),
    ("mvs_pyramid_downsample_device", _i, [_vp, _vp, _vp, _i]),
    ("mvs_pyramid_stage", _i, [_vp, _vp]),
    ("mvs_pyramid_prior", _i, [_vp, _vp, _vp, _i]),
    ("mvs_depth_filter", _i, [_vp, _vp, _vp, _i, _i, _f, _i, C.c_uint]),
    ("mvs_depth_filtered_device", _vp, [_vp]),
    ("mvs_depth_filter_fetch", _i, [_vp, _fp]),
    ("mvs_depth_fit", _i, [_vp, _vp, _vp, _i, _i, _f, _i]),
    ("mvs_depth_fit_device", _vp, [_vp]),
    ("mvs_depth_fit_depth_device", _vp, [_vp]),
    ("mvs_depth_fit_members_device", _vp, [_vp]),
    ("mvs_depth_fit_fetch", _i, [_vp, _fp, _fp, _fp, _fp, _u8p]),
    ("mvs_depth_fit_report", _i, [_vp, C.POINTER(C.c_longlong)]),
    ("mvs_depth_fit_normals", _i, [_vp, _fp]),
    ("mvs_depth_fit_normals_device", _vp, [_vp]),
    ("mvs_depth_fit_normals_fetch", _i, [_vp, _fp]),
    ("mvs_propagate_set_slopes", _i, [_vp, _vp, _vp]),
    ("mvs_propagate_init", _i, [_vp, _vp, _i, _i, _i, _i, _i, _f, C.c_uint]),
    ("mvs_propagate_run", _i, [_vp, _i, _f, _f, _i, C.c_uint]),
    ("mvs_propagate_set_gate", _i, [_vp, _i, _vp]),
    ("mvs_propagate_set_consistency", _i, [_vp, _i, _i32p, _f, _f]),
    ("mvs_propagate_support_device", _vp, [_vp]),
    ("mvs_propagate_support_fetch", _i, [_vp, _u8p]),
    ("mvs_propagate_fetch", _i, [_vp, _fp, _fp, _fp, C.POINTER(C.c_uint32)]),
    ("mvs_propagate_depth_device", _vp, [_vp]),
    ("mvs_propagate_cost_device", _vp, [_vp]),
    ("mvs_propagate_report", _i, [_vp, C.POINTER(C.c_longlong)]),
    ("mvs_sweep_argmin_partial", _i, [_vp, _vp, _i, _i, _vp]),
    ("mvs_sweep_combine_partials", _i, [_vp, _vp, _i]),
    ("mvs_sweep_volume_device", _vp, [_vp, C.POINTER(_sz)]),
    ("mvs_sweep_use_volume", _i, [_vp, _vp, _sz]),
    ("mvs_sweep_depth_device", _vp, [_vp]),
    ("mvs_sweep_cost_device", _vp, [_vp]),
    ("mvs_sweep_index_device", _vp, [_vp]),
    ("mvs_sweep_fetch", _i, [_vp, _fp, _fp, _i32p, _u32p]),
    ("mvs_sweep_view_matrices", _i, [_vp, _fp]),
    ("mvs_comm_create", _vp, [C.POINTER(_i), _i, _i, _i]),
    ("mvs_comm_destroy", None, [_vp]),
    ("mvs_comm_size", _i, [_vp]),
    ("mvs_comm_context", _vp, [_vp, _i]),
    ("mvs_comm_last_error", C.c_char_p, [_vp]),
    ("mvs_comm_set_mode", _i, [_vp, _i]),
    ("mvs_comm_mode", _i, [_vp]),
    ("mvs_comm_set_plane_groups", _i, [_vp, _i]),
    ("mvs_comm_set_planes", _i, [_vp, _i, _f, _f]),
    ("mvs_comm_set_main", _i, [_vp, _fp, _u8p]),
    ("mvs_comm_set_views", _i, [_vp, _i, _fp, C.POINTER(_u8p)]),
    ("mvs_comm_run", _i, [_vp, C.c_uint]),
    ("mvs_comm_fetch", _i, [_vp, _fp, _fp]),
    ("mvs_comm_run_async", _i, [_vp, C.c_uint]),
    ("mvs_comm_wait", _i, [_vp]),
    ("mvs_comm_pending", _i, [_vp]),
    ("mvs_comm_peer_access", _i, [_vp, _i]),
    ("mvs_comm_device", _i, [_vp, _i]),
    ("mvs_sweep_set_plan_cache", _i, [_vp, _i]),
    ("mvs_sweep_sharded", _i, [_vp, _fp, _u8p, _i, _fp, C.POINTER(_u8p), _i, _f, _f, _fp, _fp]),
    ("mvs_profile_enable", _i, [_vp, _i]),
    ("mvs_profile_read", _i, [_vp, _fp, C.POINTER(_i), _i]),
    ("mvs_device_info", C.c_char_p, [_vp]),
    ("mvs_poisson_warmup", _i, [_i]),
    ("mvs_poisson_surface", _i, [_vp, _vp, _i, _i, _f, _i, _vp]),
    ("mvs_poisson_surface_ex", _i, [_vp, _vp, _i, _i, _f, _f, _i, _vp]),
    ("mvs_surface_support", _i, [_vp, _vp]),
    ("mvs_surface_normal_scale", _i, [_vp, _vp]),
    ("mvs_surface_counts", _i, [_vp, _vp, _vp]),
    ("mvs_surface_fetch", _i, [_vp, _vp, _vp]),
    ("mvs_surface_grid", _i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("mvs_surface_spacing", _i, [_vp, _vp, _vp, _vp]),
    ("mvs_surface_enforce_criteria", _i, [_vp, _f, _f, _f, _vp]),
    ("mvs_surface_simplify", _i, [_vp, _f, _f, _vp]),
    ("mvs_surface_from_mesh", _i, [_vp, _i, _vp, _i, _f, _vp]),
    ("mvs_surface_free", None, [_vp]),
    ("mvs_surface_last_error", C.c_char_p, []),
]

_lib = None


class MvsError(RuntimeError):
    pass


def load_library(path=None):
    """dlopen libmvs_hip.so and bind every declared symbol; raises if the library or a symbol is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or os.environ.get("MVS_HIP_LIBRARY") or LIB_PATH   # MVS_HIP_LIBRARY: A/B timing of two builds in one GPU session (tools/)
    if not os.path.exists(path):
        raise MvsError(
            "HIP extension %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback)" % path)
    lib = C.CDLL(path)
    for name, res, args in ABI:
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    # test hook, not part of mvs.h
    if hasattr(lib, "mvs_test_rcp"):
        lib.mvs_test_rcp.restype = _i
        lib.mvs_test_rcp.argtypes = [_vp, C.c_uint, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    if hasattr(lib, "mvs_test_onecall_bands"):
        lib.mvs_test_onecall_bands.restype = _i
        lib.mvs_test_onecall_bands.argtypes = [_vp]
    if hasattr(lib, "mvs_test_raycast_plain"):
        lib.mvs_test_raycast_plain.restype = _i
        lib.mvs_test_raycast_plain.argtypes = [_vp, _i]
    _lib = lib
    return lib


_host_lib = None


def alpha_shape_faces(points, forced_alpha=0.0):
    """alphaShapeFaces (recon.hpp:33-34) through libmvs_host.so (host code, no GPU): points N x 3 or N x 4 (homogeneous)
    -> (faces F x 3 int32 of row indices, normals out of the solid; the alpha chosen; solid components at that alpha)"""
    global _host_lib
    if _host_lib is None:
        load_library()  # libmvs_host.so links libmvs_hip.so
        path = os.path.join(os.path.dirname(LIB_PATH), "libmvs_host.so")
        if not os.path.exists(path):
            raise MvsError("host library %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'`" % path)
        _host_lib = C.CDLL(path)
        _host_lib.mvs_alpha_shape_faces.restype = _i
        _host_lib.mvs_alpha_shape_faces.argtypes = [_vp, _i, _i, _f, _vp, _i, _vp, _vp, _vp]
    pts = np.ascontiguousarray(points, np.float32)
    if pts.ndim != 2 or pts.shape[1] not in (3, 4):
        raise ValueError("points must be N x 3 or N x 4")
    count, alpha, comps = C.c_int(), C.c_float(), C.c_int()
    rc = _host_lib.mvs_alpha_shape_faces(pts.ctypes.data_as(_vp), pts.shape[0], pts.shape[1], float(forced_alpha), None, 0, C.byref(count), C.byref(alpha), C.byref(comps))
    if rc != 0:
        raise MvsError("mvs_alpha_shape_faces failed (%d)" % rc)
    faces = np.zeros((count.value, 3), np.int32)
    rc = _host_lib.mvs_alpha_shape_faces(pts.ctypes.data_as(_vp), pts.shape[0], pts.shape[1], float(forced_alpha), faces.ctypes.data_as(_vp), count.value, C.byref(count),
                                         C.byref(alpha), C.byref(comps))
    if rc != 0:
        raise MvsError("mvs_alpha_shape_faces failed (%d)" % rc)
    return faces, alpha.value, comps.value


class CriteriaReport(C.Structure):
    """mvs_criteria_report (include/mvs.h)"""
    _fields_ = [("collapses", C.c_int), ("flips", C.c_int), ("facets_below_angle", C.c_int), ("facets_above_radius", C.c_int),
                ("min_angle_deg", C.c_float), ("max_circumradius", C.c_float), ("facets_trimmed", C.c_int)]


# cgal_poisson.cpp:50-52: sm_angle (degrees), sm_radius and sm_distance (in average spacings)
REFERENCE_FACET_CRITERIA = (20.0, 300.0, 0.375)


POISSON_SUPPORT_DEFAULT = 8.0   # MVS_POISSON_SUPPORT_DEFAULT (include/mvs.h)


def poisson_surface(points, normals, grid_log2=0, smooth_cells=1.0, criteria=REFERENCE_FACET_CRITERIA, report=None, support_spacings=POISSON_SUPPORT_DEFAULT,
                    use_precision=False, simplify=True):
    """poissonSurface (recon.hpp:37) through mvs_poisson_surface + mvs_surface_enforce_criteria: points N x 4 homogeneous, normals N x 3
    (out of the solid) -> (vertices V x 4 float32 with w = 1, faces F x 3 int32).  criteria = (min angle in degrees, max facet radius and
    max facet distance in units of the samples' average spacing), the reference's by default; None: the surface-nets mesh as it is.
    support_spacings: the level set is meshed only within that many average spacings of the samples (0: everywhere; include/mvs.h).
    use_precision: keep the normals' lengths as confidences -- what BOTH backends of the reference do (cgal_poisson.cpp:58-69 hands them to
    CGAL as they are; pcl.cpp:23 defines USE_PRECISION, so pcl.cpp:198-202 sets setConfidence(true)).  The default, False, normalises them to
    unit length first: a deliberate divergence from the reference, measured on the pipeline's own clouds (host/poisson.cpp).
    simplify (with criteria): after the criteria pass, remove the vertices the criteria do not need (mvs_surface_simplify: edge collapses under
    the same angle bound and an accumulated distance of at most criteria[2] spacings) -- the reference's mesher returns as few facets as the
    curvature allows, the grid mesher the grid's density; False: the criteria pass's mesh as it is.
    report: a dict that receives the fields of mvs_criteria_report, the average spacing, the support radius in nodes and, under "simplify",
    the fields of mvs_simplify_report"""
    lib = load_library()
    pts = np.ascontiguousarray(points, np.float32)
    nrm = np.ascontiguousarray(normals, np.float32)
    if pts.ndim != 2 or pts.shape[1] != 4 or nrm.shape != (len(pts), 3):
        raise ValueError("points must be N x 4 and normals N x 3")
    if not use_precision:
        with np.errstate(invalid="ignore", over="ignore"):
            length = np.sqrt((nrm.astype(np.float64) ** 2).sum(1))
            ok = (length > 0.0) & (length < 1e30)
        nrm = np.where(ok[:, None], nrm.astype(np.float64) / np.where(ok, length, 1.0)[:, None], nrm).astype(np.float32)
    s = C.c_void_p()
    if lib.mvs_poisson_surface_ex(pts.ctypes.data_as(_vp), nrm.ctypes.data_as(_vp), len(pts), int(grid_log2), float(smooth_cells), float(support_spacings), 0,
                                  C.byref(s)) != 0:
        raise MvsError(lib.mvs_surface_last_error().decode())
    try:
        spacing = C.c_float()
        lib.mvs_surface_spacing(s, C.byref(spacing), None, None)
        if criteria is not None and spacing.value > 0.0:
            rep = CriteriaReport()
            rc = lib.mvs_surface_enforce_criteria(s, float(criteria[0]), float(criteria[1]) * spacing.value, float(criteria[2]) * spacing.value, C.byref(rep))
            if rc != 0:
                raise MvsError("mvs_surface_enforce_criteria failed (%d)" % rc)
            if report is not None:
                report.update({name: getattr(rep, name) for name, _ in CriteriaReport._fields_})
            if simplify:
                srep = SimplifyReport()
                rc = lib.mvs_surface_simplify(s, float(criteria[0]), float(criteria[2]) * spacing.value, C.byref(srep))
                if rc != 0:
                    raise MvsError("mvs_surface_simplify failed (%d)" % rc)
                if report is not None:
                    report["simplify"] = {name: getattr(srep, name) for name, _ in SimplifyReport._fields_}
        if report is not None:
            nodes = C.c_int()
            lib.mvs_surface_support(s, C.byref(nodes))
            report["average_spacing"] = spacing.value
            report["support_nodes"] = nodes.value
        nv, nf = C.c_int(), C.c_int()
        lib.mvs_surface_counts(s, C.byref(nv), C.byref(nf))
        v = np.zeros((nv.value, 4), np.float32)
        f = np.zeros((nf.value, 3), np.int32)
        lib.mvs_surface_fetch(s, v.ctypes.data_as(_vp), f.ctypes.data_as(_vp))
    finally:
        lib.mvs_surface_free(s)
    return v, f


class SimplifyReport(C.Structure):
    _fields_ = [("collapses", C.c_int), ("vertices_before", C.c_int), ("vertices_after", C.c_int), ("facets_before", C.c_int), ("facets_after", C.c_int),
                ("max_accumulated_distance", C.c_float)]


def simplify_surface(vertices, faces, average_spacing, criteria=REFERENCE_FACET_CRITERIA):
    """mvs_surface_from_mesh + mvs_surface_simplify on a caller's mesh (host code, no GPU): -> (vertices, faces, report dict)"""
    lib = load_library()
    v = np.ascontiguousarray(vertices, np.float32)
    f = np.ascontiguousarray(faces, np.int32)
    s = C.c_void_p()
    if lib.mvs_surface_from_mesh(v.ctypes.data_as(_vp), len(v), f.ctypes.data_as(_vp), len(f), float(average_spacing), C.byref(s)) != 0:
        raise MvsError("mvs_surface_from_mesh failed")
    try:
        rep = SimplifyReport()
        rc = lib.mvs_surface_simplify(s, float(criteria[0]), float(criteria[2]) * average_spacing, C.byref(rep))
        if rc != 0:
            raise MvsError("mvs_surface_simplify failed (%d)" % rc)
        nv, nf = C.c_int(), C.c_int()
        lib.mvs_surface_counts(s, C.byref(nv), C.byref(nf))
        vo = np.zeros((nv.value, 4), np.float32)
        fo = np.zeros((nf.value, 3), np.int32)
        lib.mvs_surface_fetch(s, vo.ctypes.data_as(_vp), fo.ctypes.data_as(_vp))
        return vo, fo, {name: getattr(rep, name) for name, _ in SimplifyReport._fields_}
    finally:
        lib.mvs_surface_free(s)


def enforce_facet_criteria(vertices, faces, average_spacing, criteria=REFERENCE_FACET_CRITERIA):
    """mvs_surface_from_mesh + mvs_surface_enforce_criteria on a caller's mesh (host code, no GPU): -> (vertices, faces, report dict)"""
    lib = load_library()
    v = np.ascontiguousarray(vertices, np.float32)
    f = np.ascontiguousarray(faces, np.int32)
    if v.ndim != 2 or v.shape[1] != 4 or f.ndim != 2 or f.shape[1] != 3:
        raise ValueError("vertices must be V x 4 and faces F x 3")
    s = C.c_void_p()
    if lib.mvs_surface_from_mesh(v.ctypes.data_as(_vp), len(v), f.ctypes.data_as(_vp), len(f), float(average_spacing), C.byref(s)) != 0:
        raise MvsError("mvs_surface_from_mesh: bad argument")
    try:
        rep = CriteriaReport()
        rc = lib.mvs_surface_enforce_criteria(s, float(criteria[0]), float(criteria[1]) * average_spacing, float(criteria[2]) * average_spacing, C.byref(rep))
        if rc != 0:
            raise MvsError("mvs_surface_enforce_criteria failed (%d)" % rc)
        nv, nf = C.c_int(), C.c_int()
        lib.mvs_surface_counts(s, C.byref(nv), C.byref(nf))
        v2 = np.zeros((nv.value, 4), np.float32)
        f2 = np.zeros((nf.value, 3), np.int32)
        lib.mvs_surface_fetch(s, v2.ctypes.data_as(_vp), f2.ctypes.data_as(_vp))
    finally:
        lib.mvs_surface_free(s)
    return v2, f2, {name: getattr(rep, name) for name, _ in CriteriaReport._fields_}


def _f32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if shape is not None:
        assert a.shape == tuple(shape), (a.shape, shape)
    return a


def _u8(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if shape is not None:
        assert a.shape == tuple(shape), (a.shape, shape)
    return a


def _ptr(a, t):
    return a.ctypes.data_as(t)


class _DeviceArray:
    """minimal __cuda_array_interface__ carrier so torch can alias a library-owned device buffer without a copy"""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2,
                                         "strides": None}


def pinned_array(shape, dtype):
    """numpy array on page-locked host memory from mvs_host_alloc (freed when the array and its views are gone)"""
    lib = load_library()
    dtype = np.dtype(dtype)
    n = int(np.prod(shape)) * dtype.itemsize
    ptr = lib.mvs_host_alloc(max(n, 1))
    if not ptr:
        raise MvsError("mvs_host_alloc(%d) failed" % n)
    buf = (C.c_char * max(n, 1)).from_address(ptr)
    arr = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
    import weakref
    weakref.finalize(buf, lib.mvs_host_free, ptr)
    return arr


def _filter_step(ctx, depth_ptr, filter, step, fetch=False):
    """the `filter` keyword of the coarse-to-fine helpers: median then mean of the map at depth_ptr, the depth gate max_steps plane steps
    of the level that selected it -> the device address of the filtered map (fetch: the map itself)"""
    unknown = set(filter) - {"radius", "tau", "max_steps"}
    if unknown:
        raise ValueError("filter: unknown keys %s (radius, tau, max_steps)" % sorted(unknown))
    out = ctx.depth_filter(depth_ptr, radius=filter.get("radius", 4), tau=filter.get("tau", 255),
                           max_step=float(np.float32(float(filter.get("max_steps", float("inf"))) * step)), fetch=fetch)
    return out if fetch else ctx.depth_filtered_pointer()


def _cost_args(cost):
    """the `cost` keyword of the coarse-to-fine helpers: dict(cost="zncc" | "absdiff", radius=, keep=) -> (MVS_COST_*, radius, keep)"""
    if "tau" in cost:
        raise ValueError("cost: no key tau: the band level has no guide gate, and a half-gated two-level run would mislead; "
                         "gate the propagation instead (propagate=dict(..., tau=)) or call Context.sweep_run_bestk_gated")
    unknown = set(cost) - {"cost", "radius", "keep"}
    if unknown:
        raise ValueError("cost: unknown keys %s (cost, radius, keep)" % sorted(unknown))
    kinds = {"zncc": MVS_COST_ZNCC, "absdiff": MVS_COST_ABSDIFF}
    if cost.get("cost", "zncc") not in kinds:
        raise ValueError("cost: %r is neither \"zncc\" nor \"absdiff\"" % (cost.get("cost"),))
    return kinds[cost.get("cost", "zncc")], int(cost.get("radius", 2)), int(cost.get("keep", MVS_KEEP_ALL))


def _propagate_step(ctx, depth_ptr, propagate, cost, step, fetch):
    """the `propagate` keyword of the coarse-to-fine helpers: propagate_init + propagate_run on the map at depth_ptr with the windowed cost
    `cost` = (MVS_COST_*, radius, keep); the random steps are dz_steps / dg_steps plane steps `step` of the level that selected the map
    -> the z map (fetch) or None (it stays at propagate_depth_pointer())"""
    unknown = set(propagate) - {"iterations", "dz_steps", "dg_steps", "nrandom", "seed", "slopes", "tau", "consistency", "fit"}
    if unknown:
        raise ValueError("propagate: unknown keys %s (iterations, dz_steps, dg_steps, nrandom, seed, slopes, tau, consistency, fit)" % sorted(unknown))
    if cost is None:
        raise ValueError("propagate: needs cost=dict(cost=, radius=, keep=), the windowed cost it evaluates its hypotheses with")
    consistency = propagate.get("consistency")
    if consistency is not None:
        unknown = set(consistency) - {"slots", "weight", "max_px"}
        if unknown:
            raise ValueError("propagate: consistency: unknown keys %s (slots, weight, max_px)" % sorted(unknown))
    fit = propagate.get("fit")
    if fit is not None:
        unknown = set(fit) - {"radius", "tau", "max_steps", "min_members"}
        if unknown:
            raise ValueError("propagate: fit: unknown keys %s (radius, tau, max_steps, min_members)" % sorted(unknown))
        if propagate.get("slopes", False):
            raise ValueError("propagate: fit with slopes=True: one source of slope seeds only")

    def init():
        if fit is None:
            ctx.propagate_init(depth_ptr, *cost, slopes=bool(propagate.get("slopes", False)))
            return
        # the plane fit's slopes as seeds: the map is fitted, the depth gate max_steps plane steps of its level, the
        # slopes are recorded and the init consumes them; a refused init leaves the record, so it is cleared here
        ctx.depth_fit(depth_ptr, radius=fit.get("radius", 4), tau=fit.get("tau", 255), max_step=float(np.float32(float(fit.get("max_steps", float("inf"))) * step)),
                      min_members=fit.get("min_members", 6), fetch=False)
        maps, plane = ctx.depth_fit_pointers()[0], 4 * ctx.W * ctx.H
        try:
            ctx.propagate_set_slopes(maps + plane, maps + 2 * plane)
            ctx.propagate_init(depth_ptr, *cost)
        finally:
            ctx.propagate_set_slopes(None, None)

    if "tau" in propagate or consistency is not None:
        # the guide gate (the guide the staged main image) and the geometric term (section 27): init takes what is
        # recorded, so the defaults go back at once
        try:
            if "tau" in propagate:
                ctx.propagate_set_gate(int(propagate["tau"]))
            if consistency is not None:
                ctx.propagate_set_consistency(**consistency)
            init()
        finally:
            if "tau" in propagate:
                ctx.propagate_set_gate(255)
            if consistency is not None:
                ctx.propagate_set_consistency(())
    else:
        init()
    ctx.propagate_run(int(propagate.get("iterations", 3)), float(np.float32(float(propagate.get("dz_steps", 0.5)) * step)),
                      float(np.float32(float(propagate.get("dg_steps", 0.125)) * step)), int(propagate.get("nrandom", 2)), int(propagate.get("seed", 0)))
    return ctx.propagate_fetch()[0] if fetch else None


def coarse_to_fine(ctx, coarse_planes, band_planes, band_steps=1.5, z_lo=-1.0, z_hi=1.0, fetch=True, filter=None, cost=None, propagate=None):
    """Two-level sweep on the inputs staged on `ctx` (main view and side views; fixed sampler): `coarse_planes` planes over [z_lo, z_hi],
    refined; then `band_planes` planes within +- band_steps coarse steps of that map (mvs_sweep_run_band with the context's own depth map
    as the prior), refined and resolved.  Pure composition of Context calls -> the absolute depth map (H, W) float32 (fetch=False: None,
    the map stays on the device: sweep_band_pointers()[0]); the context is left
    with the band's plane table, volume and maps (the depth map holds offsets), and sweep_band_report() tells how the band fared.  A wrong
    coarse depth confines the band to the wrong place: this lowers the median error, not the outliers.
    filter: None, or dict(radius=, tau=, max_steps=): the coarse map is filtered (Context.depth_filter, median then mean, the guide the
    staged main image) before it becomes the band's prior, and so is the resolved map; the depth gate is max_steps plane steps of the
    level that selected the map.  The filtered resolved map is returned (fetch=False: it stays at depth_filtered_pointer()).
    cost: None (the calls above), or dict(cost="zncc" | "absdiff", radius=2, keep=MVS_KEEP_ALL): the windowed matching cost of both
    levels: the coarse level runs sweep_run_bestk, the band level sweep_run_band_bestk; "zncc" is the one for
    frames whose exposure drifts.  Use it WITH filter=: every window member is sampled at its own prior, so an outlier of a raw coarse
    map spoils the windows of its neighbours too.  On the exposure scene at 160 x 100 (ZNCC, radius 3, bad = more than 1.5 steps of a
    48-plane table off): 48 global ZNCC planes 1.06 % bad; 16 + 32 planes on the raw prior 3.7 %, on the filtered prior 0.14 %,
    what 128 global planes give.
    propagate: None (the calls above), or dict(iterations=3, dz_steps=0.5, dg_steps=0.125, nrandom=2, seed=0, slopes=False), which needs
    cost=: the map that would be returned becomes the start of Context.propagate_init / propagate_run with that cost (DESIGN.md section
    25; the random steps in plane steps of the band level), and the propagated z map is returned in its place (fetch=False: it stays at
    propagate_depth_pointer()).  It replaces outliers by their neighbours' hypotheses.  WARNING: it does not help beside depth steps: a
    window across a step prefers the nearer surface and propagation spreads that preference (on section 22's occluder scene the bad share
    of the edge pixels does not fall, and random steps of a coarse plane step raise it).  The optional key tau=0..255 gates the
    propagation's windows on the staged main image (Context.propagate_set_gate before the init, 255 restored after it; DESIGN.md section
    26): the gated propagation does repair the edge pixels of a map an ungated sweep made, wherever the step is an intensity edge.
    cost=dict(..., tau=) raises ValueError: the band level has no gate.  The optional key consistency=dict(slots=, weight=, max_px=)
    adds the geometric term against neighbour maps in the depth store (Context.propagate_set_consistency before the init, off again
    after it; DESIGN.md section 27, with its warning: consistently wrong neighbours confirm each other).  The optional key
    fit=dict(radius=4, tau=255, max_steps=inf, min_members=6) seeds the slopes with the plane fit of the start map (Context.depth_fit,
    the depth gate max_steps plane steps of the band level, then Context.propagate_set_slopes) instead of zeros;
    not together with slopes=True."""
    flags = MVS_SWEEP_VOLUME | MVS_SWEEP_FUSED_ARGMIN
    if propagate is not None and cost is None:
        raise ValueError("propagate: needs cost=dict(cost=, radius=, keep=), the windowed cost it evaluates its hypotheses with")
    ctx.sweep_set_planes(coarse_planes, z_lo, z_hi)
    if cost is None:
        ctx.sweep_run(0, None, flags)
    else:
        cost = _cost_args(cost)
        ctx.sweep_run_bestk(*cost, 0, None, flags)
    ctx.sweep_refine_depth()
    prior = ctx.sweep_result_pointers()[0]
    if filter is not None:
        prior = _filter_step(ctx, prior, filter, (float(z_hi) - float(z_lo)) / coarse_planes)
    hb = float(np.float32(band_steps * (float(z_hi) - float(z_lo)) / coarse_planes))
    ctx.sweep_set_planes(band_planes, -hb, hb)
    if cost is None:
        ctx.sweep_run_band(prior, 0, None, flags)
    else:
        ctx.sweep_run_band_bestk(prior, *cost, 0, None, flags)
    ctx.sweep_refine_depth()
    if propagate is not None:
        ctx.sweep_band_resolve(fetch=False)
        final = ctx.sweep_band_pointers()[0]
        if filter is not None:
            final = _filter_step(ctx, final, filter, 2.0 * hb / band_planes)
        return _propagate_step(ctx, final, propagate, cost, 2.0 * hb / band_planes, fetch)
    if filter is None:
        return ctx.sweep_band_resolve(fetch=fetch)
    ctx.sweep_band_resolve(fetch=False)
    out = _filter_step(ctx, ctx.sweep_band_pointers()[0], filter, 2.0 * hb / band_planes, fetch=fetch)
    return out if fetch else None


def pyramid_coarse_to_fine(ctxs, coarse_planes, band_planes, band_steps=1.5, z_lo=-1.0, z_hi=1.0, tau=255, fetch=True, filter=None, cost=None, propagate=None):
    """Coarse-to-fine over a resolution pyramid: ctxs = [fine, half] or [fine, half, quarter], each level a context
    of exactly half the size of the one before it, on one GPU, with the inputs staged on ctxs[0].  Stages down the chain (pyramid_stage);
    coarsest level: `coarse_planes` planes over [z_lo, z_hi], refined; each finer level: its prior from the level below (pyramid_prior with
    `tau`), then `band_planes` planes within +- band_steps plane steps of the level below (a band level's step is its band width over
    band_planes), refined and resolved.  Pure composition of Context calls, like coarse_to_fine -> the finest level's absolute depth map
    (H, W) float32 (fetch=False: None, the map stays on the device: ctxs[0].sweep_band_pointers()[0]); every level is left with its own
    plane table, volume and maps.
    filter: None, or dict(radius=, tau=, max_steps=): each level's upsampled prior is filtered on that level (Context.depth_filter, median
    then mean, the guide the level's staged main image) before its band run, and so is the finest level's resolved map, which is then what
    is returned (fetch=False: it stays at ctxs[0].depth_filtered_pointer()); the depth gate is max_steps plane steps of the level that
    selected the map.
    cost: None (the calls above), or dict(cost="zncc" | "absdiff", radius=2, keep=MVS_KEEP_ALL) as in coarse_to_fine: the coarsest level
    runs sweep_run_bestk and every band level sweep_run_band_bestk, the radius in pixels of each level.  As there, a raw prior makes the
    windowed band worse than the global windowed sweep (3.7 % against 1.06 % bad pixels on the exposure scene): use it with filter=.
    propagate: None (the calls above), or dict(iterations=, dz_steps=, dg_steps=, nrandom=, seed=, slopes=) as in coarse_to_fine, which
    needs cost=: the finest level's final map becomes the start of ctxs[0].propagate_init / propagate_run and the propagated z map is
    returned in its place (fetch=False: it stays at ctxs[0].propagate_depth_pointer()).  WARNING, as there: propagation does not help
    beside depth steps, where a window prefers the nearer surface; it spreads that preference -- unless it is gated with the optional
    key tau=, as there.  The optional key consistency=dict(slots=, weight=, max_px=) adds section 27's geometric term on ctxs[0], as
    there, and the optional key fit=dict(radius=, tau=, max_steps=, min_members=) seeds the slopes with section 32's plane fit, as there."""
    flags = MVS_SWEEP_VOLUME | MVS_SWEEP_FUSED_ARGMIN
    if propagate is not None and cost is None:
        raise ValueError("propagate: needs cost=dict(cost=, radius=, keep=), the windowed cost it evaluates its hypotheses with")
    for above, below in zip(ctxs, ctxs[1:]):
        above.pyramid_stage(below)
    ctxs[-1].sweep_set_planes(coarse_planes, z_lo, z_hi)
    if cost is None:
        ctxs[-1].sweep_run(0, None, flags)
    else:
        cost = _cost_args(cost)
        ctxs[-1].sweep_run_bestk(*cost, 0, None, flags)
    ctxs[-1].sweep_refine_depth()
    step = (float(z_hi) - float(z_lo)) / coarse_planes
    depth_ptr, out = None, None            # None: the depth map of the level below
    for level in range(len(ctxs) - 2, -1, -1):
        ctx = ctxs[level]
        ctx.pyramid_prior(ctxs[level + 1], depth_ptr, tau)
        prior = ctx.sweep_band_pointers()[1]
        if filter is not None:
            prior = _filter_step(ctx, prior, filter, step)
        hb = float(np.float32(band_steps * step))
        ctx.sweep_set_planes(band_planes, -hb, hb)
        if cost is None:
            ctx.sweep_run_band(prior, 0, None, flags)
        else:
            ctx.sweep_run_band_bestk(prior, *cost, 0, None, flags)
        ctx.sweep_refine_depth()
        out = ctx.sweep_band_resolve(fetch=fetch and level == 0 and filter is None and propagate is None)
        depth_ptr = ctx.sweep_band_pointers()[0]
        step = 2.0 * hb / band_planes
    if filter is not None and len(ctxs) > 1:
        out = _filter_step(ctxs[0], depth_ptr, filter, step, fetch=fetch and propagate is None)
        out = out if fetch and propagate is None else None
        depth_ptr = ctxs[0].depth_filtered_pointer()
    if propagate is not None:
        if depth_ptr is None:
            depth_ptr = ctxs[0].sweep_result_pointers()[0]      # one level: the refined global sweep's map
        out = _propagate_step(ctxs[0], depth_ptr, propagate, cost, step, fetch)
    return out


def propagate_two_stage(ctx, main_slots, main_cams, side_slots, side_cams, coarse_planes, z_lo=-1.0, z_hi=1.0, cost=None, propagate=None,
                        consistency=None, fetch=True, support=False, normals=False):
    """Geometric propagation over frames of the frame store: main_slots [n] frame-store slots with their cameras
    main_cams [n,4,4]; side_slots [n,S] and side_cams [n,S,4,4] the side views of each.  The depth store must have 2 n slots
    (Context.depth_store); nothing else is allocated beyond what the calls below allocate.
    Stage 1, for every main frame i: Context.sweep_handles stages its views, sweep_run_bestk with cost=dict(cost=, radius=, keep=) over
    `coarse_planes` planes of [z_lo, z_hi], refined, then the photometric propagation of propagate=dict(iterations=, dz_steps=,
    dg_steps=, nrandom=, seed=, slopes=, tau=) as in coarse_to_fine (the steps in coarse plane steps); its z and cost maps go device to
    device into depth slot i.
    Stage 2, for every main frame i: the term consistency=dict(weight=, max_px=) on the stage-1 slots of those of its side views that
    are main frames themselves, propagate_init from its own slot i, propagate_run; the z and cost maps go into slot n + i.
    support=True: behind the upload of slot n + i its support map (how many of those neighbours confirm each pixel) goes device to device
    into that slot's support plane (Context.depth_support_upload_device), for fuse_depth / fuse_sequence / tsdf_integrate with min_support.
    normals=True: behind the upload of slot n + i the frame's normals (Context.propagate_normals of its camera) go
    device to device into that slot's normal plane, for fuse_depth with min_normal_cos.
    normals="fit": behind the upload of each stage's slot the normals of the plane fit of that stage's final z map (Context.depth_fit with
    its defaults, then Context.depth_fit_normals of the frame's camera) go into that slot's normal plane instead.
    The term (and the gate) are off again on return -> the n stage-2 z maps [n,H,W] float32 (fetch=False: None, they are in the slots).
    WARNING: the neighbours' maps are estimated the same way as the map they correct: consistently wrong neighbours confirm each other,
    and the gain at depth steps is small (section 27 has the figures)."""
    if cost is None:
        raise ValueError("propagate_two_stage: needs cost=dict(cost=, radius=, keep=), the windowed cost of the sweep and the propagation")
    propagate = dict(propagate or {})
    if "consistency" in propagate:
        raise ValueError("propagate_two_stage: the term goes into consistency=dict(weight=, max_px=); its slots are the stage-1 slots")
    consistency = dict(consistency or {})
    unknown = set(consistency) - {"weight", "max_px"}
    if unknown:
        raise ValueError("consistency: unknown keys %s (weight, max_px)" % sorted(unknown))
    ms = [int(s) for s in np.asarray(main_slots).reshape(-1)]
    n = len(ms)
    ss = np.asarray(side_slots, dtype=np.int32).reshape(n, -1)
    mc = np.asarray(main_cams, dtype=np.float32).reshape(n, 4, 4)
    sc = np.asarray(side_cams, dtype=np.float32).reshape(n, ss.shape[1], 4, 4)
    cost = _cost_args(cost)
    step = (float(z_hi) - float(z_lo)) / coarse_planes
    out = np.empty((n, ctx.H, ctx.W), np.float32) if fetch else None
    for stage in (0, 1):
        for i in range(n):
            ctx.sweep_handles(ms[i], mc[i], ss[i], sc[i], coarse_planes, z_lo, z_hi)
            if stage == 0:
                ctx.sweep_run_bestk(*cost, 0, None, MVS_SWEEP_VOLUME | MVS_SWEEP_FUSED_ARGMIN)
                ctx.sweep_refine_depth()
                _propagate_step(ctx, ctx.sweep_result_pointers()[0], propagate, cost, step, False)
            else:
                slots = [ms.index(int(s)) for s in ss[i] if int(s) in ms]
                _propagate_step(ctx, ctx.depth_slot_pointer(i), dict(propagate, consistency=dict(consistency, slots=slots)), cost, step, False)
                if fetch:
                    out[i] = ctx.propagate_fetch()[0]
            ctx.depth_upload_device(stage * n + i, mc[i], ctx.propagate_depth_pointer(), ctx.propagate_cost_pointer())
            if support and stage == 1:
                ctx.depth_support_upload_device(n + i, ctx.propagate_support_pointer())
            if normals == "fit":
                # the plane fit of the stage's final z map (section 32): both stages' slots get a plane, unfitted pixels none
                ctx.depth_fit(ctx.propagate_depth_pointer(), fetch=False)
                ctx.depth_normals_upload_device(stage * n + i, ctx.depth_fit_normals(mc[i], fetch=False))
            elif normals and stage == 1:
                ctx.depth_normals_upload_device(n + i, ctx.propagate_normals(mc[i], fetch=False))
    return out


class Comm:
    """mvs_comm: one main view swept on several GPUs of one node (row bands by default; the views split with RCCL on request)."""

    def __init__(self, devices, width, height, sampler=None):
        self.lib = load_library()
        self.W, self.H = int(width), int(height)
        devs = (C.c_int * max(len(devices), 1))(*devices)
        self.h = self.lib.mvs_comm_create(devs if len(devices) else None, len(devices), self.W, self.H)
        if not self.h:
            raise MvsError("mvs_comm_create failed: %s" % self.lib.mvs_comm_last_error(None).decode())
        if sampler is not None:
            for r in range(self.size()):
                rc = self.lib.mvs_sweep_set_sampler(self.lib.mvs_comm_context(self.h, r), SAMPLERS[sampler])
                if rc:
                    raise MvsError("mvs_sweep_set_sampler failed on rank %d" % r)

    def size(self):
        return self.lib.mvs_comm_size(self.h)

    def set_mode(self, mode, plane_groups=None):
        """"rows" (default: row bands, no collective), "views" (plane-group all-reduce pipeline) or "views_scatter" (reduce-scatter)"""
        rc = self.lib.mvs_comm_set_mode(self.h, SHARD_MODES[mode] if isinstance(mode, str) else int(mode))
        if rc == 0 and plane_groups is not None:
            rc = self.lib.mvs_comm_set_plane_groups(self.h, int(plane_groups))
        if rc:
            raise MvsError("libmvs_hip error %d: %s" % (rc, self.lib.mvs_comm_last_error(self.h).decode()))

    def mode(self):
        return self.lib.mvs_comm_mode(self.h)

    def close(self):
        if getattr(self, "h", None):
            self.lib.mvs_comm_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sweep(self, main_cam, main_img, side_cams, side_imgs, nplanes, z_lo=-1.0, z_hi=1.0):
        W, H = self.W, self.H
        V = len(side_imgs)
        cam = _f32(main_cam, (4, 4))
        img = _u8(main_img, (H, W))
        cams = _f32(np.asarray(side_cams, dtype=np.float32).reshape(V, 4, 4)) if V else np.zeros((1, 4, 4), np.float32)
        frames = [_u8(s, (H, W)) for s in side_imgs]
        arr = (_u8p * max(V, 1))(*[_ptr(f, _u8p) for f in frames])
        depth = np.empty((H, W), np.float32)
        cost = np.empty((H, W), np.float32)
        rc = self.lib.mvs_sweep_sharded(self.h, _ptr(cam, _fp), _ptr(img, _u8p), V, _ptr(cams, _fp), arr, int(nplanes), float(z_lo), float(z_hi),
                                        _ptr(depth, _fp), _ptr(cost, _fp))
        if rc:
            raise MvsError("libmvs_hip error %d: %s" % (rc, self.lib.mvs_comm_last_error(self.h).decode()))
        return depth, cost

    def _check(self, rc):
        if rc:
            raise MvsError("libmvs_hip error %d: %s" % (rc, self.lib.mvs_comm_last_error(self.h).decode()))

    def context(self, rank):
        """the borrowed mvs_ctx handle of a rank (for the C entry points that take one)"""
        return self.lib.mvs_comm_context(self.h, int(rank))

    def set(self, main_cam, main_img, side_cams, side_imgs, nplanes, z_lo=-1.0, z_hi=1.0):
        """the resident form: planes, main view and ALL side views uploaded to every rank once (mvs_comm_set_planes / _set_main / _set_views)"""
        W, H = self.W, self.H
        V = len(side_imgs)
        cam = _f32(main_cam, (4, 4))
        img = _u8(main_img, (H, W))
        cams = _f32(np.asarray(side_cams, dtype=np.float32).reshape(V, 4, 4)) if V else np.zeros((1, 4, 4), np.float32)
        frames = [_u8(s, (H, W)) for s in side_imgs]
        arr = (_u8p * max(V, 1))(*[_ptr(f, _u8p) for f in frames])
        self._check(self.lib.mvs_comm_set_planes(self.h, int(nplanes), float(z_lo), float(z_hi)))
        self._check(self.lib.mvs_comm_set_main(self.h, _ptr(cam, _fp), _ptr(img, _u8p)))
        self._check(self.lib.mvs_comm_set_views(self.h, V, _ptr(cams, _fp), arr))

    def run(self, flags=0):
        """one sweep of what is resident in the current mode; the maps stay on rank 0's GPU (mvs_comm_run)"""
        self._check(self.lib.mvs_comm_run(self.h, int(flags)))

    def run_async(self):
        """queue one sweep of what is resident (mvs_comm_run_async): up to two in flight in rows mode; wait() publishes the oldest"""
        self._check(self.lib.mvs_comm_run_async(self.h, 0))

    def wait(self):
        self._check(self.lib.mvs_comm_wait(self.h))

    def pending(self):
        return self.lib.mvs_comm_pending(self.h)

    def peer_access(self):
        """per rank: 1 = its band copies travel GPU to GPU to rank 0, 0 = staged through host memory (mvs_comm_peer_access)"""
        return [self.lib.mvs_comm_peer_access(self.h, r) for r in range(self.size())]

    def devices(self):
        return [self.lib.mvs_comm_device(self.h, r) for r in range(self.size())]

    def note(self):
        """mvs_comm_last_error: after creation, "no error" or the note naming ranks without peer access"""
        return self.lib.mvs_comm_last_error(self.h).decode()

    def fetch(self, want_cost=True):
        depth = np.empty((self.H, self.W), np.float32)
        cost = np.empty((self.H, self.W), np.float32) if want_cost else None
        self._check(self.lib.mvs_comm_fetch(self.h, _ptr(depth, _fp), _ptr(cost, _fp) if want_cost else None))
        return (depth, cost) if want_cost else depth


class Context:
    """One GPU context (mvs_ctx).  Mirrors the life cycle of the reference's RenderGLX (render_glx.cpp:152-227)."""

    def __init__(self, width, height, device=0, sampler=None):
        self.lib = load_library()
        self.W, self.H = int(width), int(height)
        self.h = self.lib.mvs_create(int(device), self.W, self.H)
        if not self.h:
            raise MvsError("mvs_create failed: %s" % self.lib.mvs_last_error(None).decode())
        if sampler is not None:
            self.set_sampler(sampler)

    def set_sampler(self, sampler):
        """"fixed" (default of the library: 1/32-texel positions, 8-bit weight table, cells count<<24 | sum) or "exact"
        (f32 bilinear rounded to u8, cells count<<16 | sum) -- include/mvs.h"""
        self._check(self.lib.mvs_sweep_set_sampler(self.h, SAMPLERS[sampler] if isinstance(sampler, str) else int(sampler)))

    def sampler(self):
        return {v: k for k, v in SAMPLERS.items()}[self.lib.mvs_sweep_sampler(self.h)]

    def close(self):
        if getattr(self, "h", None):
            self.lib.mvs_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise MvsError("libmvs_hip error %d: %s" % (rc, self.lib.mvs_last_error(self.h).decode()))

    def info(self):
        return self.lib.mvs_device_info(self.h).decode()

    def synchronize(self):
        self._check(self.lib.mvs_synchronize(self.h))

    def set_stream(self, stream_handle):
        self._check(self.lib.mvs_set_stream(self.h, C.c_void_p(stream_handle)))

    # ---- sweep ----------------------------------------------------------------------------------
    def sweep(self, main_cam, main_img, side_cams, side_imgs, nplanes, z_lo=-1.0, z_hi=1.0, want_cost=False,
              want_volume=False):
        """mvs_sweep on host buffers -> depth (H,W) [, cost (H,W)] [, volume (D,H,W)]"""
        W, H = self.W, self.H
        V = len(side_imgs)
        cam = _f32(main_cam, (4, 4))
        img = _u8(main_img, (H, W))
        cams = _f32(np.asarray(side_cams, dtype=np.float32).reshape(V, 4, 4)) if V else np.zeros((0, 4, 4), np.float32)
        frames = [_u8(s, (H, W)) for s in side_imgs]
        arr = (_u8p * max(V, 1))(*[_ptr(f, _u8p) for f in frames])
        depth = np.empty((H, W), np.float32)
        cost = np.empty((H, W), np.float32) if want_cost else None
        vol = np.empty((nplanes, H, W), np.float32) if want_volume else None
        self.D = int(nplanes)   # the views and planes stay resident: sweep_run / sweep_fetch may follow
        self._check(self.lib.mvs_sweep(self.h, _ptr(cam, _fp), _ptr(img, _u8p), V, _ptr(cams, _fp), arr, int(nplanes),
                                       float(z_lo), float(z_hi), _ptr(depth, _fp),
                                       _ptr(cost, _fp) if want_cost else None, _ptr(vol, _fp) if want_volume else None))
        out = [depth]
        if want_cost:
            out.append(cost)
        if want_volume:
            out.append(vol)
        return out[0] if len(out) == 1 else tuple(out)

    def warp_by_depth(self, main_cam, depth, side_cam, frame):
        cam, sc = _f32(main_cam, (4, 4)), _f32(side_cam, (4, 4))
        d, f = _f32(depth, (self.H, self.W)), _u8(frame, (self.H, self.W))
        out = np.empty((self.H, self.W, 2), np.uint8)
        self._check(self.lib.mvs_warp_by_depth(self.h, _ptr(cam, _fp), _ptr(d, _fp), _ptr(sc, _fp), _ptr(f, _u8p), _ptr(out, _u8p)))
        return out

    def sweep_set(self, main_cam, main_img, side_cams, side_imgs, nplanes, z_lo=-1.0, z_hi=1.0):
        W, H = self.W, self.H
        V = len(side_imgs)
        cam = _f32(main_cam, (4, 4))
        img = _u8(main_img, (H, W))
        self._check(self.lib.mvs_sweep_set_main(self.h, _ptr(cam, _fp), _ptr(img, _u8p)))
        cams = _f32(np.asarray(side_cams, dtype=np.float32).reshape(V, 4, 4)) if V else np.zeros((0, 4, 4), np.float32)
        frames = [_u8(s, (H, W)) for s in side_imgs]
        arr = (_u8p * max(V, 1))(*[_ptr(f, _u8p) for f in frames])
        self._check(self.lib.mvs_sweep_set_views(self.h, V, _ptr(cams, _fp), arr))
        self._check(self.lib.mvs_sweep_set_planes(self.h, int(nplanes), float(z_lo), float(z_hi)))
        self.V, self.D = V, int(nplanes)

    def sweep_set_views(self, side_cams, side_imgs):
        """mvs_sweep_set_views alone (new side views for the main view already set)"""
        W, H = self.W, self.H
        V = len(side_imgs)
        cams = _f32(np.asarray(side_cams, dtype=np.float32).reshape(V, 4, 4)) if V else np.zeros((0, 4, 4), np.float32)
        frames = [_u8(s, (H, W)) for s in side_imgs]
        arr = (_u8p * max(V, 1))(*[_ptr(f, _u8p) for f in frames])
        self._check(self.lib.mvs_sweep_set_views(self.h, V, _ptr(cams, _fp), arr))
        self.V = V

    def sweep_set_planes(self, nplanes, z_lo=-1.0, z_hi=1.0):
        self._check(self.lib.mvs_sweep_set_planes(self.h, int(nplanes), float(z_lo), float(z_hi)))
        self.D = int(nplanes)

    def sweep_set_main(self, main_cam, main_img):
        """mvs_sweep_set_main alone: the main camera and its H*W u8 image (the default guide of sweep_window)"""
        cam = _f32(main_cam, (4, 4))
        img = _u8(main_img, (self.H, self.W))
        self._check(self.lib.mvs_sweep_set_main(self.h, _ptr(cam, _fp), _ptr(img, _u8p)))

    def sweep_set_main_device(self, main_cam, main_ptr):
        """mvs_sweep_set_main_device: main_ptr = address of H*W u8 in the memory of the context's GPU (e.g. tensor.data_ptr()); stream-ordered"""
        cam = _f32(main_cam, (4, 4))
        self._check(self.lib.mvs_sweep_set_main_device(self.h, _ptr(cam, _fp), C.c_void_p(int(main_ptr))))

    def sweep_set_views_device(self, side_cams, side_ptrs):
        """mvs_sweep_set_views_device: side_ptrs = device addresses of the side frames (H*W u8 each); stream-ordered, no synchronisation"""
        V = len(side_ptrs)
        cams = _f32(np.asarray(side_cams, dtype=np.float32).reshape(V, 4, 4)) if V else np.zeros((0, 4, 4), np.float32)
        arr = (_vp * max(V, 1))(*[C.c_void_p(int(q)) for q in side_ptrs])
        self._check(self.lib.mvs_sweep_set_views_device(self.h, V, _ptr(cams, _fp), arr))
        self.V = V

    def sweep_run(self, view_first=0, view_count=None, flags=MVS_SWEEP_VOLUME):
        if view_count is None:
            view_count = self.V - view_first
        self._check(self.lib.mvs_sweep_run(self.h, int(view_first), int(view_count), int(flags)))

    def sweep_run_planes(self, view_first, view_count, plane_first, plane_count, flags=MVS_SWEEP_VOLUME):
        self._check(self.lib.mvs_sweep_run_planes(self.h, int(view_first), int(view_count), int(plane_first), int(plane_count),
                                                  int(flags)))

    def plane_granularity(self):
        return self.lib.mvs_sweep_plane_granularity()

    def sweep_run_rows(self, row_first, row_count, view_first=0, view_count=None, flags=MVS_SWEEP_VOLUME):
        if view_count is None:
            view_count = self.V - view_first
        self._check(self.lib.mvs_sweep_run_rows(self.h, int(view_first), int(view_count), int(row_first), int(row_count), int(flags)))

    def row_granularity(self):
        """row-band boundaries must be multiples of this (depends on the sampler set on the context)"""
        return self.lib.mvs_sweep_row_granularity_of(self.h)

    def set_plan_cache(self, enable):
        self._check(self.lib.mvs_sweep_set_plan_cache(self.h, 1 if enable else 0))

    def plan_shape(self):
        return self.lib.mvs_sweep_plan_shape(self.h)

    def sweep_refine_depth(self):
        """sub-plane parabola refinement of the depth map (needs the volume and a depth selection of the same run)"""
        self._check(self.lib.mvs_sweep_refine_depth(self.h))

    # ---- frame store + batched sweep (a sequence on one GPU) ------------------------------------
    def frame_store(self, capacity):
        self._check(self.lib.mvs_frame_store(self.h, int(capacity)))
        self._store_keep = {}

    def frame_upload(self, slot, frame, lens=False):
        """mvs_frame_upload; lens=True: mvs_frame_upload_lens (the frame goes through the context's lens on its way into the slot)"""
        f = _u8(frame, (self.H, self.W))
        self._store_keep[int(slot)] = f   # the copy is asynchronous: keep the array alive until the next synchronising call
        self._check((self.lib.mvs_frame_upload_lens if lens else self.lib.mvs_frame_upload)(self.h, int(slot), f.ctypes.data_as(C.c_void_p)))

    def frame_upload_device(self, slot, frame_ptr, lens=False):
        """mvs_frame_upload_device (lens=True: mvs_frame_upload_lens_device): frame_ptr = device address of H*W u8 (stream-ordered)"""
        self._check((self.lib.mvs_frame_upload_lens_device if lens else self.lib.mvs_frame_upload_device)(self.h, int(slot), C.c_void_p(int(frame_ptr))))

    # ---- lens: distorted frames -> pinhole frames (include/mvs.h) ---------
    def set_lens(self, k, center=None):
        """mvs_set_lens: k = up to three radial coefficients (None clears the lens); center = (center-x, center-y) in pixels, y from the
        bottom as in the tracks files (None: the frame's centre)"""
        if k is None:
            self._check(self.lib.mvs_set_lens(self.h, None, 0.0, 0.0))
            return
        kk = np.zeros(3, np.float32)
        k = np.asarray(k, np.float32).reshape(-1)
        kk[:min(3, len(k))] = k[:3]
        cx, cy = (self.W / 2.0, self.H / 2.0) if center is None else center
        self._check(self.lib.mvs_set_lens(self.h, _ptr(kk, _fp), float(cx), float(cy)))

    def lens(self):
        """mvs_lens -> (k[3], (center-x, center-y)) or None when no lens is set"""
        k = np.zeros(3, np.float32)
        cx, cy = C.c_float(), C.c_float()
        rc = self.lib.mvs_lens(self.h, _ptr(k, _fp), C.byref(cx), C.byref(cy))
        if rc < 0:
            self._check(rc)
        return (k, (cx.value, cy.value)) if rc else None

    def undistort(self, frame):
        """mvs_undistort: one H x W u8 frame through the lens"""
        f = _u8(frame, (self.H, self.W))
        out = np.empty((self.H, self.W), np.uint8)
        self._check(self.lib.mvs_undistort(self.h, _ptr(f, _u8p), _ptr(out, _u8p)))
        return out

    def undistort_device(self, src_ptr, dst_ptr, nframes=1):
        """mvs_undistort_device: nframes tightly packed H*W u8 frames, device addresses, one launch (stream-ordered)"""
        self._check(self.lib.mvs_undistort_device(self.h, C.c_void_p(int(src_ptr)), C.c_void_p(int(dst_ptr)), int(nframes)))

    def undistort_map(self):
        """mvs_undistort_map -> [H, W, 2] f32: the source position (x, y) of every output pixel, computed by the device"""
        out = np.empty((self.H, self.W, 2), np.float32)
        self._check(self.lib.mvs_undistort_map(self.h, _ptr(out, _fp)))
        return out

    def sweep_handles(self, main_slot, main_cam, side_slots, side_cams, nplanes, z_lo=-1.0, z_hi=1.0, want_cost=False, out=None):
        """mvs_sweep_handles: one main view whose frames are slots of the frame store -> depth [H,W] (, cost)"""
        ss = np.ascontiguousarray(side_slots, dtype=np.int32).reshape(-1)
        S = len(ss)
        mc = _f32(main_cam, (4, 4))
        sc = _f32(np.asarray(side_cams, dtype=np.float32).reshape(S, 4, 4)) if S else np.zeros((1, 4, 4), np.float32)
        depth = out if out is not None else np.empty((self.H, self.W), np.float32)
        cost = np.empty((self.H, self.W), np.float32) if want_cost else None
        self._check(self.lib.mvs_sweep_handles(self.h, int(main_slot), _ptr(mc, _fp), S, ss.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p), int(nplanes),
                                               float(z_lo), float(z_hi), depth.ctypes.data_as(C.c_void_p), cost.ctypes.data_as(C.c_void_p) if want_cost else None))
        self._store_keep = {}
        self.V, self.D = S, int(nplanes)
        return (depth, cost) if want_cost else depth

    def sweep_batch_async(self, main_slots, main_cams, side_slots, side_cams, nplanes, out, z_lo=-1.0, z_hi=1.0, cost_out=None):
        """mvs_sweep_batch_async: queues the batch; `out` [M,H,W] f32 (page-locked: pinned_array) is complete after sweep_batch_wait()"""
        ms = np.ascontiguousarray(main_slots, dtype=np.int32)
        ss = np.ascontiguousarray(side_slots, dtype=np.int32)
        M, S = ss.shape
        mc = _f32(np.asarray(main_cams, dtype=np.float32).reshape(M, 4, 4))
        sc = _f32(np.asarray(side_cams, dtype=np.float32).reshape(M, S, 4, 4))
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.size >= M * self.H * self.W
        assert cost_out is None or (cost_out.dtype == np.float32 and cost_out.flags.c_contiguous and cost_out.size >= M * self.H * self.W)
        # the copy stream writes into these arrays after this call has returned: they stay referenced until the wait (a caller that
        # drops its page-locked array -- mvs_host_free through the finalizer -- would hand the DMA freed memory: ADVICE r04)
        if not hasattr(self, "_batch_keep"):
            self._batch_keep = []
        self._batch_keep.append((out, cost_out))
        # the library keeps two batches in flight and waits for the oldest itself when a third is queued (batch_slot[2]): the arrays of
        # anything older are complete and need no reference from here (a caller that never calls the wait would otherwise pin them all)
        del self._batch_keep[:-2]
        self._check(self.lib.mvs_sweep_batch_async(self.h, M, ms.ctypes.data_as(C.c_void_p), mc.ctypes.data_as(C.c_void_p), S, ss.ctypes.data_as(C.c_void_p),
                                                   sc.ctypes.data_as(C.c_void_p), int(nplanes), float(z_lo), float(z_hi), out.ctypes.data_as(C.c_void_p),
                                                   cost_out.ctypes.data_as(C.c_void_p) if cost_out is not None else None))

    def sweep_batch_wait(self):
        try:
            self._check(self.lib.mvs_sweep_batch_wait(self.h))
        finally:
            self._batch_keep = []

    def sweep_batch(self, main_slots, main_cams, side_slots, side_cams, nplanes, z_lo=-1.0, z_hi=1.0, want_cost=False, out=None):
        """mvs_sweep_batch: main_slots [M], main_cams [M,4,4], side_slots [M,S], side_cams [M,S,4,4] -> depth [M,H,W] (, cost [M,H,W])"""
        ms = np.ascontiguousarray(main_slots, dtype=np.int32)
        ss = np.ascontiguousarray(side_slots, dtype=np.int32)
        M, S = ss.shape
        mc = _f32(np.asarray(main_cams, dtype=np.float32).reshape(M, 4, 4))
        sc = _f32(np.asarray(side_cams, dtype=np.float32).reshape(M, S, 4, 4))
        depth = out if out is not None else np.empty((M, self.H, self.W), np.float32)
        cost = np.empty((M, self.H, self.W), np.float32) if want_cost else None
        self._check(self.lib.mvs_sweep_batch(self.h, M, ms.ctypes.data_as(C.c_void_p), mc.ctypes.data_as(C.c_void_p), S, ss.ctypes.data_as(C.c_void_p),
                                             sc.ctypes.data_as(C.c_void_p), int(nplanes), float(z_lo), float(z_hi), depth.ctypes.data_as(C.c_void_p),
                                             cost.ctypes.data_as(C.c_void_p) if want_cost else None))
        self._store_keep = {}
        return (depth, cost) if want_cost else depth

    # ---- depth store + fusion ---------------------------------------------------------------------
    def depth_store(self, capacity):
        """mvs_depth_store: capacity slots of H*W depth + cost + camera; re-sizing empties the store"""
        self._check(self.lib.mvs_depth_store(self.h, int(capacity)))
        self._depth_keep = {}

    def depth_upload(self, slot, cam, depth, cost=None):
        """mvs_depth_upload: depth [H,W] f32 NDC z (1.0 = empty), cost [H,W] f32 or None (asynchronous: the arrays are kept alive here
        until the next fuse_depth)"""
        c = _f32(cam, (4, 4))
        d = _f32(depth, (self.H, self.W))
        k = _f32(cost, (self.H, self.W)) if cost is not None else None
        self.__dict__.setdefault("_depth_keep", {})[int(slot)] = (c, d, k)
        self._check(self.lib.mvs_depth_upload(self.h, int(slot), _ptr(c, _fp), _ptr(d, _fp), _ptr(k, _fp) if k is not None else None))

    def depth_upload_device(self, slot, cam, depth_ptr, cost_ptr=None):
        """mvs_depth_upload_device: device addresses of H*W f32 depth (and cost), e.g. sweep_result_pointers() (stream-ordered)"""
        c = _f32(cam, (4, 4))
        self._check(self.lib.mvs_depth_upload_device(self.h, int(slot), _ptr(c, _fp), C.c_void_p(int(depth_ptr)),
                                                     C.c_void_p(int(cost_ptr)) if cost_ptr else None))

    def depth_support_upload(self, slot, support):
        """mvs_depth_support_upload: support [H,W] u8, the support plane of a filled depth slot (asynchronous: the array is kept alive here
        until the next fuse_depth / fuse_sequence)"""
        s = np.ascontiguousarray(np.asarray(support, dtype=np.uint8).reshape(self.H, self.W))
        self.__dict__.setdefault("_depth_keep", {})[("support", int(slot))] = s
        self._check(self.lib.mvs_depth_support_upload(self.h, int(slot), _ptr(s, _u8p)))

    def depth_support_upload_device(self, slot, ptr):
        """mvs_depth_support_upload_device: the device address of H*W u8, e.g. propagate_support_pointer() (stream-ordered)"""
        self._check(self.lib.mvs_depth_support_upload_device(self.h, int(slot), C.c_void_p(int(ptr)) if ptr else None))

    def depth_support_fetch(self, slot):
        """mvs_depth_support_fetch -> (H, W) uint8, the slot's support plane; synchronises"""
        out = np.empty((self.H, self.W), np.uint8)
        self._check(self.lib.mvs_depth_support_fetch(self.h, int(slot), _ptr(out, _u8p)))
        return out

    def depth_support_drop(self, slot):
        """mvs_depth_support_drop: the slot has no support plane any more (its depth map stays)"""
        self._check(self.lib.mvs_depth_support_drop(self.h, int(slot)))

    def depth_normals_upload(self, slot, normals):
        """mvs_depth_normals_upload: normals [H,W,3] f32 (unit, zeros = none), the normal plane of a filled depth slot (asynchronous: the
        array is kept alive here until the next fuse_depth / fuse_sequence)"""
        s = _f32(normals, (self.H, self.W, 3))
        self.__dict__.setdefault("_depth_keep", {})[("normals", int(slot))] = s
        self._check(self.lib.mvs_depth_normals_upload(self.h, int(slot), _ptr(s, _fp)))

    def depth_normals_upload_device(self, slot, ptr):
        """mvs_depth_normals_upload_device: the device address of H*W*3 f32, e.g. propagate_normals_pointer() or tsdf_raycast's normals
        (stream-ordered)"""
        self._check(self.lib.mvs_depth_normals_upload_device(self.h, int(slot), C.c_void_p(int(ptr)) if ptr else None))

    def depth_normals_fetch(self, slot):
        """mvs_depth_normals_fetch -> (H, W, 3) float32, the slot's normal plane; synchronises"""
        out = np.empty((self.H, self.W, 3), np.float32)
        self._check(self.lib.mvs_depth_normals_fetch(self.h, int(slot), _ptr(out, _fp)))
        return out

    def depth_normals_drop(self, slot):
        """mvs_depth_normals_drop: the slot has no normal plane any more (its depth map stays)"""
        self._check(self.lib.mvs_depth_normals_drop(self.h, int(slot)))

    def fuse_depth(self, ref_slot, neighbour_slots, min_consistent=2, max_reproj_px=1.0, max_rel_depth=0.01, max_cost=float("inf"), copy=True,
                   min_support=0, min_normal_cos=None):
        """mvs_fuse_depth -> (N, 7) float32 rows (x, y, z, 1, nx, ny, nz) in ascending pixel index.  copy=False: a view of the context's
        reusable output buffer (the one process_frame uses), valid until the next call that writes it.  min_support > 0:
        mvs_fuse_depth_masked, rule 1s on the slots' support planes.  min_normal_cos a number (<= 1,
        -inf = no test): mvs_fuse_depth_normals, rules 3n and 5n on the slots' normal planes (section 31)"""
        nb = np.ascontiguousarray(np.asarray(list(neighbour_slots) if len(neighbour_slots) else [0], dtype=np.int32))
        if getattr(self, "_pf_out", None) is None:
            self._pf_out = np.zeros((self.H * self.W, 7), np.float32)
        out = self._pf_out
        n = C.c_int(0)
        try:
            if min_normal_cos is not None:
                self._check(self.lib.mvs_fuse_depth_normals(self.h, int(ref_slot), len(neighbour_slots), _ptr(nb, _i32p), int(min_consistent),
                                                            float(max_reproj_px), float(max_rel_depth), float(max_cost), int(min_support),
                                                            float(min_normal_cos), _ptr(out, _fp), C.byref(n)))
            elif int(min_support):
                self._check(self.lib.mvs_fuse_depth_masked(self.h, int(ref_slot), len(neighbour_slots), _ptr(nb, _i32p), int(min_consistent),
                                                           float(max_reproj_px), float(max_rel_depth), float(max_cost), int(min_support), _ptr(out, _fp),
                                                           C.byref(n)))
            else:
                self._check(self.lib.mvs_fuse_depth(self.h, int(ref_slot), len(neighbour_slots), _ptr(nb, _i32p), int(min_consistent), float(max_reproj_px),
                                                    float(max_rel_depth), float(max_cost), _ptr(out, _fp), C.byref(n)))
        finally:
            self._depth_keep = {}
        return out[:n.value].copy() if copy else out[:n.value]

    def fuse_sequence(self, ref_slots, neighbour_slots, min_consistent=2, max_reproj_px=1.0, max_rel_depth=0.01, max_cost=float("inf"), min_support=0,
                      max_rows=None, copy=True):
        """mvs_fuse_sequence -> (rows (N, 7) float32, ref_counts [nrefs] int32): the references fused in list order, every surface point
        once.  neighbour_slots: one list per reference; ragged lists are padded with -1.  max_rows=None makes a
        counting call first and then the exact one; otherwise at most max_rows rows come back (ref_counts and their sum are the totals
        either way).  copy=False: the rows stay on the device (fuse_sequence_points_device()) and rows is None."""
        refs = np.ascontiguousarray(np.asarray(list(ref_slots), dtype=np.int32).reshape(-1))
        lists = [[int(s) for s in row] for row in neighbour_slots]
        if len(lists) != len(refs):
            raise ValueError("fuse_sequence: one neighbour list per reference")
        K = max([len(row) for row in lists] + [0])
        nb = np.full((max(len(refs), 1), max(K, 1)), -1, np.int32)
        for i, row in enumerate(lists):
            nb[i, :len(row)] = row
        nb = np.ascontiguousarray(nb[:, :K]) if K else nb
        counts = np.zeros(max(len(refs), 1), np.int32)
        total = C.c_longlong(0)

        def call(rows_max, out):
            self._check(self.lib.mvs_fuse_sequence(self.h, len(refs), _ptr(refs, _i32p), K, _ptr(nb, _i32p), int(min_consistent), float(max_reproj_px),
                                                   float(max_rel_depth), float(max_cost), int(min_support), int(rows_max),
                                                   _ptr(out, _fp) if out is not None else None, _ptr(counts, _i32p), C.byref(total)))

        try:
            if max_rows is None:
                call(0, None)
                max_rows = total.value
            out = np.zeros((min(int(max_rows), len(refs) * self.H * self.W), 7), np.float32) if copy and int(max_rows) > 0 else None
            call(max_rows, out)
        finally:
            self._depth_keep = {}
        if not copy:
            return None, counts[:len(refs)].copy()
        n = min(total.value, int(max_rows))
        return (out[:n] if out is not None else np.zeros((0, 7), np.float32)), counts[:len(refs)].copy()

    def fuse_sequence_points_device(self):
        """device address of the rows of the last fuse_sequence (0 before the first)"""
        return self.lib.mvs_fuse_sequence_points_device(self.h) or 0

    def fuse_points_device(self):
        """device address of the rows of the last fuse_depth (0 before the first)"""
        return self.lib.mvs_fuse_points_device(self.h) or 0

    def depth_slot_matrices(self, slot):
        """mvs_depth_slot_matrices -> (P [4,4], P^-1 [4,4], centre [4]) as the fusion kernels use them"""
        m = np.empty(36, np.float32)
        self._check(self.lib.mvs_depth_slot_matrices(self.h, int(slot), _ptr(m, _fp)))
        return m[:16].reshape(4, 4).copy(), m[16:32].reshape(4, 4).copy(), m[32:].copy()

    # ---- TSDF fusion -------------------------------------------------------------------------------
    def tsdf_volume(self, nodes_per_axis, origin, node_spacing, truncation):
        """mvs_tsdf_volume: a cleared G^3 volume, node (i, j, k) at origin + node_spacing (i, j, k); again: cleared"""
        o = _f32(origin, (3,))
        self._check(self.lib.mvs_tsdf_volume(self.h, int(nodes_per_axis), _ptr(o, _fp), float(node_spacing), float(truncation)))
        self._tsdf_G = int(nodes_per_axis)

    def tsdf_integrate(self, slots, max_cost=float("inf"), min_support=0):
        """mvs_tsdf_integrate: add the listed depth-store slots' maps, in list order (asynchronous, stream-ordered).  min_support > 0:
        mvs_tsdf_integrate_masked, rule 1s on the slots' support planes"""
        sl = np.ascontiguousarray(np.asarray(list(slots) if len(slots) else [0], dtype=np.int32))
        if int(min_support):
            self._check(self.lib.mvs_tsdf_integrate_masked(self.h, len(slots), _ptr(sl, _i32p), None, float(max_cost), int(min_support)))
        else:
            self._check(self.lib.mvs_tsdf_integrate(self.h, len(slots), _ptr(sl, _i32p), float(max_cost)))

    def tsdf_fetch(self):
        """mvs_tsdf_fetch -> (sum [G, G, G] f32, count [G, G, G] i32), indexed [k][j][i]"""
        G = getattr(self, "_tsdf_G", 0)
        if not G:   # no volume made through this object: the library's answer (MVS_ESTATE before mvs_tsdf_volume)
            self._check(self.lib.mvs_tsdf_fetch(self.h, None, None))
            raise MvsError("tsdf_fetch: the volume was not made with tsdf_volume")
        s = np.empty((G, G, G), np.float32)
        c = np.empty((G, G, G), np.int32)
        try:
            self._check(self.lib.mvs_tsdf_fetch(self.h, _ptr(s, _fp), _ptr(c, _i32p)))
        finally:
            self._depth_keep = {}
        return s, c

    def tsdf_surface(self, min_observations=1):
        """mvs_tsdf_surface -> (vertices N x 4 f32 with w = 1, faces F x 3 i32 facing the cameras); the surface is freed here"""
        s = C.c_void_p()
        try:
            self._check(self.lib.mvs_tsdf_surface(self.h, int(min_observations), C.byref(s)))
        finally:
            self._depth_keep = {}
        try:
            nv, nf = C.c_int(), C.c_int()
            self.lib.mvs_surface_counts(s, C.byref(nv), C.byref(nf))
            v = np.zeros((nv.value, 4), np.float32)
            f = np.zeros((nf.value, 3), np.int32)
            self.lib.mvs_surface_fetch(s, v.ctypes.data_as(_vp), f.ctypes.data_as(_vp))
        finally:
            self.lib.mvs_surface_free(s)
        return v, f

    def tsdf_upload(self, sdf_sum, count):
        """mvs_tsdf_upload: replace the volume's fields by sum [G, G, G] f32 and count [G, G, G] i32, indexed [k][j][i] (synchronises)"""
        G = getattr(self, "_tsdf_G", 0)
        if not G:   # no volume made through this object: the library's answer (MVS_ESTATE before mvs_tsdf_volume)
            one_f, one_i = np.zeros(1, np.float32), np.zeros(1, np.int32)
            self._check(self.lib.mvs_tsdf_upload(self.h, _ptr(one_f, _fp), _ptr(one_i, _i32p)))
            raise MvsError("tsdf_upload: the volume was not made with tsdf_volume")
        s = _f32(sdf_sum, (G, G, G))
        c = np.ascontiguousarray(count, np.int32)
        if c.shape != (G, G, G):
            raise ValueError("count must be [%d, %d, %d]" % (G, G, G))
        try:
            self._check(self.lib.mvs_tsdf_upload(self.h, _ptr(s, _fp), _ptr(c, _i32p)))
        finally:
            self._depth_keep = {}

    def tsdf_raycast(self, cam, min_observations=1, step=0.5, fetch=True):
        """mvs_tsdf_raycast: the volume's zero level set as seen by `cam` -> (depth [H, W] f32 NDC z, 1.0 = empty; normals [H, W, 3] f32,
        unit, zeros = empty).  step: the march's step in node spacings (keep it <= truncation / (2 h)).  fetch=False: queue the raycast only
        (asynchronous; the maps stay on the device: tsdf_raycast_pointers) and return None"""
        c = _f32(cam, (4, 4))
        self._check(self.lib.mvs_tsdf_raycast(self.h, _ptr(c, _fp), int(min_observations), float(step)))
        if not fetch:
            return None
        d = np.empty((self.H, self.W), np.float32)
        n = np.empty((self.H, self.W, 3), np.float32)
        try:
            self._check(self.lib.mvs_tsdf_raycast_fetch(self.h, _ptr(d, _fp), _ptr(n, _fp)))
        finally:
            self._depth_keep = {}
        return d, n

    def tsdf_raycast_pointers(self):
        """device addresses (depth H*W f32, normals H*W*3 f32) of the last raycast; (0, 0) before the first"""
        return self.lib.mvs_tsdf_raycast_depth_device(self.h) or 0, self.lib.mvs_tsdf_raycast_normals_device(self.h) or 0

    # ---- appearance of the TSDF volume --------------------------------------------------------------
    def tsdf_integrate_frames(self, depth_slots, frame_slots, max_cost=float("inf"), min_support=0):
        """mvs_tsdf_integrate_frames: mvs_tsdf_integrate of depth_slots, and frame-store slot frame_slots[e] votes its intensities into the
        appearance volume along with depth_slots[e] (asynchronous, stream-ordered).  min_support > 0: mvs_tsdf_integrate_masked"""
        if len(depth_slots) != len(frame_slots):
            raise ValueError("depth_slots and frame_slots must pair up")
        ds = np.ascontiguousarray(np.asarray(list(depth_slots) if len(depth_slots) else [0], dtype=np.int32))
        fs = np.ascontiguousarray(np.asarray(list(frame_slots) if len(frame_slots) else [0], dtype=np.int32))
        if int(min_support):
            self._check(self.lib.mvs_tsdf_integrate_masked(self.h, len(depth_slots), _ptr(ds, _i32p), _ptr(fs, _i32p), float(max_cost), int(min_support)))
        else:
            self._check(self.lib.mvs_tsdf_integrate_frames(self.h, len(depth_slots), _ptr(ds, _i32p), _ptr(fs, _i32p), float(max_cost)))

    def tsdf_appearance_fetch(self):
        """mvs_tsdf_appearance_fetch -> cells [G, G, G] u32 (count << 24 | sum), indexed [k][j][i]"""
        G = getattr(self, "_tsdf_G", 0)
        if not G:
            raise MvsError("tsdf_appearance_fetch: the volume was not made with tsdf_volume")
        cells = np.empty((G, G, G), np.uint32)
        try:
            self._check(self.lib.mvs_tsdf_appearance_fetch(self.h, _ptr(cells, _u32p)))
        finally:
            self._depth_keep = {}
        return cells

    def tsdf_appearance_upload(self, cells):
        """mvs_tsdf_appearance_upload: replace the appearance volume by cells [G, G, G] u32, indexed [k][j][i] (synchronises)"""
        G = getattr(self, "_tsdf_G", 0)
        if not G:
            raise MvsError("tsdf_appearance_upload: the volume was not made with tsdf_volume")
        c = np.ascontiguousarray(cells, np.uint32)
        if c.shape != (G, G, G):
            raise ValueError("cells must be [%d, %d, %d]" % (G, G, G))
        try:
            self._check(self.lib.mvs_tsdf_appearance_upload(self.h, _ptr(c, _u32p)))
        finally:
            self._depth_keep = {}

    def tsdf_shade(self, cam, depth_ptr, fetch=True):
        """mvs_tsdf_shade: the volume's appearance at the surface points of the device depth map at address depth_ptr (H*W f32 in `cam`'s
        depth convention, e.g. tsdf_raycast_pointers()[0]) -> [H, W, 2] u8: (grey, 255), or (0, 0) where there is none.  fetch=False: queue
        the launch only (asynchronous; the map stays on the device: tsdf_shade_pointer) and return None"""
        c = _f32(cam, (4, 4))
        self._check(self.lib.mvs_tsdf_shade(self.h, _ptr(c, _fp), C.c_void_p(int(depth_ptr)) if depth_ptr else None))
        if not fetch:
            return None
        out = np.empty((self.H, self.W, 2), np.uint8)
        try:
            self._check(self.lib.mvs_tsdf_shade_fetch(self.h, _ptr(out, _u8p)))
        finally:
            self._depth_keep = {}
        return out

    def tsdf_shade_pointer(self):
        """device address of the last shaded map (H*W pairs of u8); 0 before the first"""
        return self.lib.mvs_tsdf_shade_device(self.h) or 0

    def tsdf_sample_appearance(self, points):
        """mvs_tsdf_sample_appearance: points [N, 4] rows (x, y, z, w), e.g. tsdf_surface's vertices -> [N] f32 grey levels, NaN = none"""
        p = _f32(np.asarray(points, np.float32).reshape(-1, 4))
        out = np.empty(len(p), np.float32)
        one = np.zeros(4, np.float32)
        try:
            self._check(self.lib.mvs_tsdf_sample_appearance(self.h, _ptr(p if len(p) else one, _fp), len(p), _ptr(out if len(p) else one, _fp)))
        finally:
            self._depth_keep = {}
        return out

    def depth_slot_pointer(self, slot):
        """device address of a filled depth slot's H*W f32 map (0: unfilled, or outside the store)"""
        return self.lib.mvs_depth_slot_device(self.h, int(slot)) or 0

    def depth_device_array(self):
        """zero-copy [H, W] f32 view of the device depth map for torch.as_tensor(..., device='cuda') (valid until the
        context is closed; the buffer exists after the first sweep run)"""
        ptr = self.lib.mvs_sweep_depth_device(self.h)
        if not ptr:
            raise MvsError("no depth map on the device yet")
        return _DeviceArray(ptr, (self.H, self.W), "<f4")

    def sweep_argmin(self):
        self._check(self.lib.mvs_sweep_argmin(self.h))

    def sweep_aggregate(self, paths=8, p1=16, p2=128, cost_cap=4080, refine=False):
        """mvs_sweep_aggregate: semi-global aggregation of the packed volume along 4 or 8 paths, then depth selection over the sums
        (rewrites the depth / cost / index maps; asynchronous, stream-ordered)"""
        self._check(self.lib.mvs_sweep_aggregate(self.h, int(paths), int(p1), int(p2), int(cost_cap), MVS_AGGREGATE_REFINE if refine else 0))

    def sweep_aggregate_fetch(self):
        """mvs_sweep_aggregate_fetch -> S (D, H, W) uint16 of the last sweep_aggregate (synchronises)"""
        n = _sz(0)
        self.lib.mvs_sweep_aggregated_device(self.h, C.byref(n))
        if not n.value:   # nothing aggregated yet: the library's answer (MVS_ESTATE)
            self._check(self.lib.mvs_sweep_aggregate_fetch(self.h, None))
            raise MvsError("sweep_aggregate_fetch: nothing aggregated yet")
        s = np.empty((n.value // (2 * self.H * self.W), self.H, self.W), np.uint16)
        self._check(self.lib.mvs_sweep_aggregate_fetch(self.h, _ptr(s, C.POINTER(C.c_uint16))))
        return s

    def sweep_aggregated_device(self):
        """(device address, bytes) of S, [D][H][W] uint16; raises before the first sweep_aggregate"""
        n = _sz(0)
        p = self.lib.mvs_sweep_aggregated_device(self.h, C.byref(n))
        if not p:
            raise MvsError("nothing aggregated yet (sweep_aggregate first)")
        return p, n.value

    def sweep_clean(self, min_views=0, uniqueness=0, speckle_min_size=0, speckle_max_diff=1, aggregated=False):
        """mvs_sweep_clean: reject pixels of the depth / cost / index maps by view count, uniqueness (in per cent; `aggregated`: on the
        sums of the last sweep_aggregate) and component size (asynchronous, stream-ordered)"""
        self._check(self.lib.mvs_sweep_clean(self.h, int(min_views), int(uniqueness), int(speckle_min_size), int(speckle_max_diff),
                                             MVS_CLEAN_SCORES_AGGREGATED if aggregated else 0))

    def sweep_clean_report(self):
        """mvs_sweep_clean_report -> [pixels with an index before the last sweep_clean, rejected by rule 1, 2, 3] (synchronises)"""
        out = (C.c_int * 4)()
        self._check(self.lib.mvs_sweep_clean_report(self.h, out))
        return list(out)

    def sweep_clean_sizes(self):
        """mvs_sweep_clean_sizes_fetch -> (H, W) int32 component sizes of the last sweep_clean's speckle filter (synchronises)"""
        sizes = np.empty((self.H, self.W), np.int32)
        self._check(self.lib.mvs_sweep_clean_sizes_fetch(self.h, _ptr(sizes, _i32p)))
        return sizes

    def sweep_window(self, radius=2, tau=255, guide_ptr=None, select=True, refine=False):
        """mvs_sweep_window: the windowed volume Wv of the packed volume -- per cell the mean cost over the (2 radius + 1)^2 window, taking
        only the neighbours whose guide value is within `tau` of the pixel's (guide_ptr: device address of H*W uint8, None = the staged
        main image; tau 255 = plain box); `select` also rewrites the depth / cost / index maps from Wv, `refine` with the parabola
        (asynchronous, stream-ordered)"""
        flags = (MVS_WINDOW_SELECT if select else 0) | (MVS_WINDOW_REFINE if refine else 0)
        self._check(self.lib.mvs_sweep_window(self.h, int(radius), int(tau), C.c_void_p(guide_ptr) if guide_ptr else None, flags))

    def sweep_window_fetch(self):
        """mvs_sweep_window_fetch -> Wv (D, H, W) uint32 of the last sweep_window (synchronises)"""
        n = _sz(0)
        self.lib.mvs_sweep_windowed_device(self.h, C.byref(n))
        if not n.value:   # no window yet: the library's answer (MVS_ESTATE)
            self._check(self.lib.mvs_sweep_window_fetch(self.h, (C.c_uint32 * 1)()))
            raise MvsError("sweep_window_fetch: no windowed volume yet")
        cells = np.empty((n.value // (4 * self.H * self.W), self.H, self.W), np.uint32)
        self._check(self.lib.mvs_sweep_window_fetch(self.h, _ptr(cells, _u32p)))
        return cells

    def sweep_windowed_device(self):
        """(device address, bytes) of Wv, [D][H][W] uint32; raises before the first sweep_window"""
        n = _sz(0)
        p = self.lib.mvs_sweep_windowed_device(self.h, C.byref(n))
        if not p:
            raise MvsError("no windowed volume yet (sweep_window first)")
        return p, n.value

    def set_volume_source(self, source):
        """mvs_sweep_set_volume_source: "raw" / "windowed" (or the constants): the packed volume sweep_argmin, sweep_refine_depth,
        sweep_aggregate and sweep_clean read"""
        self._check(self.lib.mvs_sweep_set_volume_source(self.h, VOLUME_SOURCES.get(source, source)))

    def volume_source(self):
        return self.lib.mvs_sweep_volume_source(self.h)

    def sweep_run_band(self, prior_ptr, view_first=0, view_count=None, flags=MVS_SWEEP_VOLUME | MVS_SWEEP_FUSED_ARGMIN):
        """mvs_sweep_run_band: the fixed sampler's sweep with plane d of pixel p at prior(p) + delta_d, delta = the staged plane table
        (sweep_set_planes(D, -hb, +hb)); prior_ptr: device address of H*W float32, e.g. sweep_result_pointers()[0].  The depth map holds
        OFFSETS until sweep_band_resolve (asynchronous, stream-ordered)"""
        if view_count is None:
            view_count = self.V - view_first
        self._check(self.lib.mvs_sweep_run_band(self.h, int(view_first), int(view_count), C.c_void_p(int(prior_ptr)) if prior_ptr else None, int(flags)))

    def sweep_band_resolve(self, fetch=True):
        """mvs_sweep_band_resolve: prior + selected offset -> the absolute depth map band_depth (the depth / cost / index maps stay);
        fetch: -> (H, W) float32 (synchronises), else None (asynchronous)"""
        self._check(self.lib.mvs_sweep_band_resolve(self.h))
        if not fetch:
            return None
        depth = np.empty((self.H, self.W), np.float32)
        self._check(self.lib.mvs_sweep_band_fetch(self.h, _ptr(depth, _fp)))
        return depth

    def sweep_band_report(self):
        """mvs_sweep_band_report -> [pixels with a prior, with an index, with index 0 or D - 1, emptied by the range test] of the last
        sweep_band_resolve (synchronises)"""
        out = (C.c_int * 4)()
        self._check(self.lib.mvs_sweep_band_report(self.h, out))
        return list(out)

    def sweep_band_pointers(self):
        """(device address of band_depth, of the context's copy of the prior); 0 before the first resolve / band run"""
        return self.lib.mvs_sweep_band_depth_device(self.h) or 0, self.lib.mvs_sweep_band_prior_device(self.h) or 0

    def sweep_run_zncc(self, radius=2, view_first=0, view_count=None, flags=MVS_SWEEP_VOLUME | MVS_SWEEP_FUSED_ARGMIN):
        """mvs_sweep_run_zncc: the fixed sampler's sweep with zero-mean normalised cross-correlation over the (2 radius + 1)^2 window as
        the matching cost (radius 1..4); the same packed volume and maps as sweep_run, the cost map reads 127.5 (1 - ncc)
        (asynchronous, stream-ordered)"""
        if view_count is None:
            view_count = self.V - view_first
        self._check(self.lib.mvs_sweep_run_zncc(self.h, int(view_first), int(view_count), int(radius), int(flags)))

    def sweep_run_bestk(self, cost, radius=2, keep=2, view_first=0, view_count=None, flags=MVS_SWEEP_VOLUME | MVS_SWEEP_FUSED_ARGMIN):
        """mvs_sweep_run_bestk: the fixed sampler's sweep whose cell keeps the `keep` lowest per-view windowed costs (1..8, or MVS_KEEP_ALL)
        instead of the sum over every view, so that views in which the point is hidden drop out; cost MVS_COST_ZNCC (radius 1..4) or
        MVS_COST_ABSDIFF (radius 0..4; 0 is a cross-check, best-K of single-pixel costs is worse than the sum).  The same packed volume
        and maps as sweep_run; the volumes of disjoint view ranges do not add (asynchronous, stream-ordered)"""
        if view_count is None:
            view_count = self.V - view_first
        self._check(self.lib.mvs_sweep_run_bestk(self.h, int(view_first), int(view_count), int(cost), int(radius), int(keep), int(flags)))

    def sweep_run_bestk_gated(self, cost, radius=2, keep=2, tau=30, guide_ptr=None, view_first=0, view_count=None, flags=MVS_SWEEP_VOLUME | MVS_SWEEP_FUSED_ARGMIN):
        """mvs_sweep_run_bestk_gated: sweep_run_bestk whose window of pixel p holds only the pixels q with |G(q) - G(p)| <= tau (0..255) on
        the guide G (guide_ptr: device address of H*W uint8, None = the staged main image), so that the pixels across an intensity edge
        leave the window; radius 1..4 for both costs.  tau 255 or a constant guide gives sweep_run_bestk's bytes.  WARNING: a tau below
        the texture's own contrast starves ZNCC of variance (views stop counting) and is worse than a larger one.  The window is no
        longer separable: (2 radius + 1)^2 LDS reads per pixel, plane and view (asynchronous, stream-ordered)"""
        if view_count is None:
            view_count = self.V - view_first
        self._check(self.lib.mvs_sweep_run_bestk_gated(self.h, int(view_first), int(view_count), int(cost), int(radius), int(keep), int(tau),
                                                       C.c_void_p(int(guide_ptr)) if guide_ptr else None, int(flags)))

    def sweep_run_band_bestk(self, prior_ptr, cost, radius=2, keep=MVS_KEEP_ALL, view_first=0, view_count=None, flags=MVS_SWEEP_VOLUME | MVS_SWEEP_FUSED_ARGMIN):
        """mvs_sweep_run_band_bestk: sweep_run_bestk with plane d of pixel q at prior(q) + delta_d, delta = the staged plane table
        (sweep_set_planes(D, -hb, +hb)); every window member is sampled at its own prior.  cost MVS_COST_ZNCC (radius 1..4) or
        MVS_COST_ABSDIFF (radius 0..4), keep 1..8 or MVS_KEEP_ALL (with MVS_COST_ZNCC: the ZNCC band sweep).  prior_ptr: device address
        of H*W float32, e.g. sweep_result_pointers()[0], sweep_band_pointers()[1], depth_filtered_pointer().  It leaves the band state
        of sweep_run_band: the depth map holds OFFSETS until sweep_band_resolve.  Filter a raw coarse prior first: its outliers stay
        outliers and spoil their neighbours' windows (asynchronous, stream-ordered)"""
        if view_count is None:
            view_count = self.V - view_first
        self._check(self.lib.mvs_sweep_run_band_bestk(self.h, int(view_first), int(view_count), C.c_void_p(int(prior_ptr)) if prior_ptr else None, int(cost),
                                                      int(radius), int(keep), int(flags)))

    # ---- depth-map filter (include/mvs.h) -----------------------------------
    def depth_filter(self, depth_ptr, radius=4, tau=255, max_step=float("inf"), guide_ptr=None, median=True, mean=True, fill=0, fetch=True):
        """mvs_depth_filter: the gated median (`median`) and / or gated mean (`mean`) over the (2 radius + 1)^2 window of the H*W float32
        depth map at device address depth_ptr (sweep_result_pointers()[0], sweep_band_pointers()[0], tsdf_raycast_pointers()[0],
        depth_slot_pointer(slot), depth_filtered_pointer(), ...).  A neighbour counts when its guide value is within `tau` of the
        pixel's (guide_ptr: H*W uint8, None = the staged main image; tau 255 = no guide) and, in the mean, when its depth is within
        max_step of the pixel's (inf = no depth gate).  fill = k > 0: the median also fills an invalid pixel that has at least k valid
        members.  max_step is in depth units, a few plane steps: below the surface's own change of depth across the window it makes a
        slanted surface worse.  fetch: -> (H, W) float32 (synchronises), else None (asynchronous, stream-ordered; the map stays at
        depth_filtered_pointer())"""
        flags = (MVS_FILTER_MEDIAN if median else 0) | (MVS_FILTER_MEAN if mean else 0) | (MVS_FILTER_FILL if fill else 0)
        self._check(self.lib.mvs_depth_filter(self.h, C.c_void_p(int(depth_ptr)) if depth_ptr else None, C.c_void_p(int(guide_ptr)) if guide_ptr else None,
                                              int(radius), int(tau), float(max_step), int(fill), flags))
        if not fetch:
            return None
        depth = np.empty((self.H, self.W), np.float32)
        self._check(self.lib.mvs_depth_filter_fetch(self.h, _ptr(depth, _fp)))
        return depth

    def depth_filtered_pointer(self):
        """device address of the filtered map of the last depth_filter (0 before the first)"""
        return self.lib.mvs_depth_filtered_device(self.h) or 0

    # ---- depth-map plane fit (include/mvs.h) --------------------------------
    def depth_fit(self, depth_ptr, radius=4, tau=255, max_step=float("inf"), min_members=6, guide_ptr=None, fetch=True):
        """mvs_depth_fit: a least-squares plane through the (2 radius + 1)^2 window of every pixel of the H*W float32 depth map at device
        address depth_ptr (whatever depth_filter takes, and depth_fit_pointers()[1]).  A neighbour is a member when its guide value is
        within `tau` of the pixel's (guide_ptr: H*W uint8, None = the staged main image; tau 255 = no guide) and its depth within
        max_step of the pixel's (inf = no depth gate); a pixel is fitted when it has at least min_members (3..81) members that are not
        collinear.  fetch: -> (z, gx, gy, zfit (H, W) float32, members (H, W) uint8): the map as read, the depth's change per column and
        per row (0 unless fitted), the depth moved onto the plane, and the members of a fitted pixel (else 0); synchronises.  Else None
        (asynchronous, stream-ordered; the maps stay at depth_fit_pointers())"""
        self._check(self.lib.mvs_depth_fit(self.h, C.c_void_p(int(depth_ptr)) if depth_ptr else None, C.c_void_p(int(guide_ptr)) if guide_ptr else None,
                                           int(radius), int(tau), float(max_step), int(min_members)))
        if not fetch:
            return None
        z, gx, gy, zfit = (np.empty((self.H, self.W), np.float32) for _ in range(4))
        members = np.empty((self.H, self.W), np.uint8)
        self._check(self.lib.mvs_depth_fit_fetch(self.h, _ptr(z, _fp), _ptr(gx, _fp), _ptr(gy, _fp), _ptr(zfit, _fp), _ptr(members, _u8p)))
        return z, gx, gy, zfit, members

    def depth_fit_pointers(self):
        """device addresses (z, gx, gy: 3 * H*W float32 in propagate_depth_pointer()'s layout; zfit H*W float32, a depth map; members
        H*W uint8) of the last depth_fit; (0, 0, 0) before the first"""
        return self.lib.mvs_depth_fit_device(self.h) or 0, self.lib.mvs_depth_fit_depth_device(self.h) or 0, self.lib.mvs_depth_fit_members_device(self.h) or 0

    def depth_fit_report(self):
        """mvs_depth_fit_report -> [valid centres, fitted, refused for too few members, refused for collinear members] of the last
        depth_fit; synchronises"""
        out = (C.c_longlong * 4)()
        self._check(self.lib.mvs_depth_fit_report(self.h, out))
        return list(out)

    def depth_fit_normals(self, cam, fetch=True):
        """mvs_depth_fit_normals: world-space unit normals of the last depth_fit's planes for the main camera cam [4,4] (rule N1, DESIGN.md
        section 31; a pixel that is not fitted gets zeros) -> (H, W, 3) float32; synchronises.  fetch=False: the map's device address
        (asynchronous), which depth_normals_upload_device takes"""
        c = _f32(cam, (4, 4))
        self._check(self.lib.mvs_depth_fit_normals(self.h, _ptr(c, _fp)))
        if not fetch:
            return self.depth_fit_normals_pointer()
        out = np.empty((self.H, self.W, 3), np.float32)
        self._check(self.lib.mvs_depth_fit_normals_fetch(self.h, _ptr(out, _fp)))
        return out

    def depth_fit_normals_pointer(self):
        """device address of the fit's normal map, H*W*3 float32 (0 before the first depth_fit_normals)"""
        return self.lib.mvs_depth_fit_normals_device(self.h) or 0

    def propagate_set_slopes(self, gx_ptr, gy_ptr):
        """mvs_propagate_set_slopes: records two device addresses of H*W float32 slope maps (e.g. depth_fit_pointers()[0] + 4 H W and
        + 8 H W) that the NEXT propagate_init which passes its checks gives to the pixels with a hypothesis in place of zero slopes (a
        non-finite value as 0), and forgets: one-shot.  (None, None) clears the record.  Not together with propagate_init(slopes=True)"""
        self._check(self.lib.mvs_propagate_set_slopes(self.h, C.c_void_p(int(gx_ptr)) if gx_ptr else None, C.c_void_p(int(gy_ptr)) if gy_ptr else None))

    # ---- hypothesis propagation (include/mvs.h) ----------------------------
    def propagate_init(self, depth_ptr, cost, radius=2, keep=MVS_KEEP_ALL, view_first=0, view_count=None, slopes=False, max_step=float("inf")):
        """mvs_propagate_init: every pixel gets the hypothesis (z, gx, gy) -- z from the H*W float32 depth map at device address depth_ptr
        (sweep_result_pointers()[0], sweep_band_pointers()[0], depth_filtered_pointer(), propagate_depth_pointer(), ...), the slopes 0 or,
        with `slopes`, the map's differences between neighbours no more than max_step apart -- and the packed cell of that hypothesis
        under the windowed cost (MVS_COST_ZNCC radius 1..4, MVS_COST_ABSDIFF radius 0..4; keep 1..8 or MVS_KEEP_ALL) over the given side
        views.  Fixed sampler; no plane table is needed (asynchronous, stream-ordered)"""
        if view_count is None:
            view_count = self.V - view_first
        self._check(self.lib.mvs_propagate_init(self.h, C.c_void_p(int(depth_ptr)) if depth_ptr else None, int(view_first), int(view_count), int(cost), int(radius),
                                                int(keep), float(max_step), MVS_PROPAGATE_SLOPES if slopes else 0))

    def propagate_set_gate(self, tau, guide_ptr=None):
        """mvs_propagate_set_gate: records the guide gate the NEXT propagate_init takes (and the propagate_run calls behind it use): window
        member q of p is live only if |G(q) - G(p)| <= tau (0..255; 255, the default, is no gate) on the guide G (guide_ptr: device
        address of H*W uint8, copied by that init; None = the staged main image).  The same warning about a small tau as
        sweep_run_bestk_gated"""
        self._check(self.lib.mvs_propagate_set_gate(self.h, int(tau), C.c_void_p(int(guide_ptr)) if guide_ptr else None))

    def propagate_set_consistency(self, slots, weight=0.0, max_px=1.0):
        """mvs_propagate_set_consistency: records the geometric term the NEXT propagate_init takes (and the propagate_run calls behind
        it use).  slots: up to 8 slots of the depth store holding the neighbouring views' depth maps and cameras (read when the kernels
        run, not copied); a hypothesis pays `weight` grey levels of the cost map's scale (ZNCC: 127.5 (1 - ncc)) per pixel of forward /
        backward reprojection error against each neighbour, capped at max_px pixels and averaged over the neighbours, and
        propagate_support() counts per pixel the neighbours within max_px.  slots=() turns the term off (the default).  WARNING:
        consistently wrong neighbours confirm each other"""
        s = np.ascontiguousarray(np.asarray(list(slots), dtype=np.int32).reshape(-1))
        self._check(self.lib.mvs_propagate_set_consistency(self.h, len(s), _ptr(s, _i32p) if len(s) else None, float(weight), float(max_px)))

    def propagate_support(self, fetch=True):
        """mvs_propagate_support_fetch -> (H, W) uint8: the listed neighbours that confirm the hypothesis each pixel holds (all 0 without
        a geometric term); synchronises.  fetch=False: the map's device address (propagate_support_pointer())"""
        if not fetch:
            return self.propagate_support_pointer()
        out = np.empty((self.H, self.W), np.uint8)
        self._check(self.lib.mvs_propagate_support_fetch(self.h, _ptr(out, _u8p)))
        return out

    def propagate_support_pointer(self):
        """device address of the support map, H*W uint8 (0 before the first propagate_init)"""
        return self.lib.mvs_propagate_support_device(self.h) or 0

    def propagate_normals(self, cam, fetch=True):
        """mvs_propagate_normals: world-space unit normals of the hypotheses as they are now, for the main camera cam [4,4] (rule N1,
        DESIGN.md section 31) -> (H, W, 3) float32, zeros = none; synchronises.  fetch=False: the map's device address (asynchronous)"""
        c = _f32(cam, (4, 4))
        self._check(self.lib.mvs_propagate_normals(self.h, _ptr(c, _fp)))
        if not fetch:
            return self.propagate_normals_pointer()
        out = np.empty((self.H, self.W, 3), np.float32)
        self._check(self.lib.mvs_propagate_normals_fetch(self.h, _ptr(out, _fp)))
        return out

    def propagate_normals_pointer(self):
        """device address of the normal map, H*W*3 float32 (0 before the first propagate_normals)"""
        return self.lib.mvs_propagate_normals_device(self.h) or 0

    def propagate_run(self, iterations, dz, dg, nrandom=2, seed=0):
        """mvs_propagate_run: `iterations` PatchMatch iterations on the hypotheses of propagate_init.  In each of an iteration's two
        checkerboard halves an active pixel tests the planes of its neighbours at distance 1 and 5 and `nrandom` (0..4) perturbations of
        what it holds (depth within +-dz, slopes within +-dg, both halved every iteration) and keeps what matches better.  Outliers are
        replaced by their neighbours' hypotheses; the cost's minimum is not sharpened.  Beside depth steps it does NOT help: a window
        across a step prefers the nearer surface and propagation spreads that preference (DESIGN.md section 25 has the figures).
        run(a) then run(b) with the same arguments is run(a + b) (asynchronous, stream-ordered)"""
        self._check(self.lib.mvs_propagate_run(self.h, int(iterations), float(dz), float(dg), int(nrandom), int(seed) & 0xffffffff))

    def propagate_fetch(self):
        """mvs_propagate_fetch -> (z, gx, gy (H, W) float32, cells (H, W) uint32: k << 24 | sum); synchronises"""
        z, gx, gy = (np.empty((self.H, self.W), np.float32) for _ in range(3))
        cells = np.empty((self.H, self.W), np.uint32)
        self._check(self.lib.mvs_propagate_fetch(self.h, _ptr(z, _fp), _ptr(gx, _fp), _ptr(gy, _fp), _ptr(cells, C.POINTER(C.c_uint32))))
        return z, gx, gy, cells

    def propagate_depth_pointer(self):
        """device address of the z map, a depth map in the library's convention (0 before the first propagate_init)"""
        return self.lib.mvs_propagate_depth_device(self.h) or 0

    def propagate_cost_pointer(self):
        """device address of the mean-cost map of the cells, +inf for cell 0 (0 before the first propagate_init)"""
        return self.lib.mvs_propagate_cost_device(self.h) or 0

    def propagate_report(self):
        """mvs_propagate_report -> [kept, near, far, random since propagate_init, pixels holding a cell != 0 now]; synchronises"""
        out = (C.c_longlong * 5)()
        self._check(self.lib.mvs_propagate_report(self.h, out))
        return list(out)

    # ---- resolution pyramid (include/mvs.h) --------------------------------
    def pyramid_downsample_device(self, src_ptr, dst_ptr, nframes=1):
        """mvs_pyramid_downsample_device: nframes tightly packed H*W u8 frames -> (H/2)*(W/2) frames (rounded 2 x 2 means), device
        addresses, one launch (stream-ordered)"""
        self._check(self.lib.mvs_pyramid_downsample_device(self.h, C.c_void_p(int(src_ptr)), C.c_void_p(int(dst_ptr)), int(nframes)))

    def pyramid_stage(self, coarse):
        """mvs_pyramid_stage: stages on `coarse` (a Context of exactly half this one's size) the half-resolution copy of what is staged
        here: main image, side views, the same cameras.  The planes stay the caller's: coarse.sweep_set_planes"""
        self._check(self.lib.mvs_pyramid_stage(self.h, coarse.h))
        if hasattr(self, "V"):
            coarse.V = self.V

    def pyramid_prior(self, coarse, depth_ptr=None, tau=255):
        """mvs_pyramid_prior: the coarse level's depth map (depth_ptr: device address of (H/2)*(W/2) f32; None: coarse's own depth map)
        upsampled into this context's prior buffer, sweep_band_pointers()[1], which is returned; tau < 255 keeps to the taps whose guide
        pixel is within tau grey levels of this pixel's (the staged main images are the guides).  A new prior ends this context's band run:
        sweep_band_resolve / _report refuse until the next one"""
        self._check(self.lib.mvs_pyramid_prior(self.h, coarse.h, C.c_void_p(int(depth_ptr)) if depth_ptr else None, int(tau)))
        return self.lib.mvs_sweep_band_prior_device(self.h)

    def sweep_argmin_partial(self, volume_slice_ptr, plane_first, plane_count, partial_out_ptr):
        self._check(self.lib.mvs_sweep_argmin_partial(self.h, C.c_void_p(volume_slice_ptr), int(plane_first), int(plane_count),
                                                      C.c_void_p(partial_out_ptr)))

    def sweep_combine_partials(self, partials_ptr, nparts):
        self._check(self.lib.mvs_sweep_combine_partials(self.h, C.c_void_p(partials_ptr), int(nparts)))

    def sweep_volume_device(self):
        n = _sz(0)
        p = self.lib.mvs_sweep_volume_device(self.h, C.byref(n))
        if not p:
            raise MvsError("no volume: %s" % self.lib.mvs_last_error(self.h).decode())
        return p, n.value

    def sweep_use_volume(self, device_ptr, nbytes):
        self._check(self.lib.mvs_sweep_use_volume(self.h, C.c_void_p(device_ptr), nbytes))

    def sweep_result_pointers(self):
        return (self.lib.mvs_sweep_depth_device(self.h), self.lib.mvs_sweep_cost_device(self.h),
                self.lib.mvs_sweep_index_device(self.h))

    def sweep_fetch(self, want_volume=False):
        W, H = self.W, self.H
        depth = np.empty((H, W), np.float32)
        cost = np.empty((H, W), np.float32)
        idx = np.empty((H, W), np.int32)
        vol = np.empty((self.D, H, W), np.uint32) if want_volume else None
        self._check(self.lib.mvs_sweep_fetch(self.h, _ptr(depth, _fp), _ptr(cost, _fp), _ptr(idx, _i32p),
                                             _ptr(vol, _u32p) if want_volume else None))
        return depth, cost, idx, vol

    def sweep_view_matrices(self):
        q = np.empty((self.V, 3, 4), np.float32)
        self._check(self.lib.mvs_sweep_view_matrices(self.h, _ptr(q, _fp)))
        return q

    # ---- profiling ------------------------------------------------------------------------------
    def profile_enable(self, on=True):
        self._check(self.lib.mvs_profile_enable(self.h, 1 if on else 0))

    def profile_read(self, reset=True):
        ms = (C.c_float * MVS_K_COUNT)()
        n = (C.c_int * MVS_K_COUNT)()
        self._check(self.lib.mvs_profile_read(self.h, ms, n, 1 if reset else 0))
        return list(ms), list(n)

    # ---- renderer / helpers ---------------------------------------------------------------------
    def load_mesh(self, verts4, faces3):
        v = _f32(verts4)
        f = np.ascontiguousarray(faces3, dtype=np.int32)
        assert v.ndim == 2 and v.shape[1] == 4 and f.ndim == 2 and f.shape[1] == 3
        self._check(self.lib.mvs_load_mesh(self.h, _ptr(v, _fp), v.shape[0], _ptr(f, _i32p), f.shape[0]))

    def depth(self, cam):
        cam = _f32(cam, (4, 4))
        out = np.empty((self.H, self.W), np.float32)
        self._check(self.lib.mvs_depth(self.h, _ptr(cam, _fp), _ptr(out, _fp)))
        return out

    def depth_probe(self, cam, rows, cols):
        cam = _f32(cam, (4, 4))
        rows = np.ascontiguousarray(rows, np.int32).ravel()
        cols = np.ascontiguousarray(cols, np.int32).ravel()
        if rows.shape != cols.shape:
            raise ValueError("rows and cols differ in length")
        out = np.empty(rows.shape[0], np.float32)
        self._check(self.lib.mvs_depth_probe(self.h, _ptr(cam, _fp), rows.shape[0], _ptr(rows, _i32p), _ptr(cols, _i32p), _ptr(out, _fp)))
        return out

    def resize(self, img, dw, dh):
        """cv::resize(img, Size(dw, dh)) INTER_LINEAR on u8 (configuration.cpp:233)"""
        img = np.ascontiguousarray(img, np.uint8)
        sh, sw = img.shape[:2]
        ch = 1 if img.ndim == 2 else img.shape[2]
        out = np.empty((dh, dw) if img.ndim == 2 else (dh, dw, ch), np.uint8)
        self._check(self.lib.mvs_resize_u8(self.h, img.ctypes.data_as(C.c_void_p), sw, sh, ch, out.ctypes.data_as(C.c_void_p), int(dw), int(dh)))
        return out

    def set_texture_filter(self, name):
        """"mipmap" (default: the reference's GL_LINEAR_MIPMAP_LINEAR request) or "level0" for Render::projected's frame texture"""
        self._check(self.lib.mvs_set_texture_filter(self.h, {"mipmap": 0, "level0": 1}[name]))

    def projected(self, cam, frame, projector):
        cam = _f32(cam, (4, 4))
        prj = _f32(projector, (4, 4))
        frame = _u8(frame, (self.H, self.W))
        out = np.empty((self.H, self.W, 3), np.uint8)
        self._check(self.lib.mvs_projected(self.h, _ptr(cam, _fp), _ptr(frame, _u8p), _ptr(prj, _fp), _ptr(out, _u8p)))
        return out

    def mix_background(self, img3, bg, depth):
        img3 = _u8(img3, (self.H, self.W, 3))
        bg = _u8(bg, (self.H, self.W))
        depth = _f32(depth, (self.H, self.W)).copy()
        out = np.empty((self.H, self.W), np.uint8)
        self._check(self.lib.mvs_mix_background(self.h, _ptr(img3, _u8p), _ptr(bg, _u8p), _ptr(depth, _fp),
                                                _ptr(out, _u8p)))
        return out, depth

    def compare(self, prev, nxt):
        prev = _u8(prev, (self.H, self.W))
        nxt = _u8(nxt, (self.H, self.W))
        out = np.empty((self.H, self.W), np.float32)
        self._check(self.lib.mvs_compare(self.h, _ptr(prev, _u8p), _ptr(nxt, _u8p), _ptr(out, _fp)))
        return out

    def flow_remap(self, flow, image):
        flow = _f32(flow)
        assert flow.shape[:2] == (self.H, self.W)
        image = _u8(image, (self.H, self.W))
        out = np.empty((self.H, self.W), np.uint8)
        self._check(self.lib.mvs_flow_remap(self.h, _ptr(flow, _fp), flow.shape[2], _ptr(image, _u8p), _ptr(out, _u8p)))
        return out

    def flow(self, prev, nxt, use_farneback):
        prev = _u8(prev, (self.H, self.W))
        nxt = _u8(nxt, (self.H, self.W))
        out = np.empty((self.H, self.W, 4), np.float32)
        self._check(self.lib.mvs_flow(self.h, _ptr(prev, _u8p), _ptr(nxt, _u8p), 1 if use_farneback else 0,
                                      _ptr(out, _fp)))
        return out

    def triangulate(self, flows, main_cam, side_cams, depth, copy=True):
        """mvs_triangulate -> (N, 7) rows (x, y, z, w, nx, ny, nz) in pixel scan order (copy=False: a view of the context's
        reusable output buffer, valid until the next triangulate / process_frame call -- see process_frame)"""
        V = len(flows)
        fl = [_f32(f, (self.H, self.W, 4)) for f in flows]
        arr = (_fp * max(V, 1))(*[_ptr(f, _fp) for f in fl])
        cam = _f32(main_cam, (4, 4))
        cams = _f32(np.asarray(side_cams, dtype=np.float32).reshape(V, 4, 4)) if V else np.zeros((1, 4, 4), np.float32)
        depth = _f32(depth, (self.H, self.W))
        if getattr(self, "_pf_out", None) is None:
            self._pf_out = np.zeros((self.H * self.W, 7), np.float32)
        out = self._pf_out
        n = C.c_int(0)
        self._check(self.lib.mvs_triangulate(self.h, V, arr, _ptr(cam, _fp), _ptr(cams, _fp), _ptr(depth, _fp), _ptr(out, _fp),
                                             C.byref(n)))
        return out[:n.value].copy() if copy else out[:n.value]

    def process_frame(self, main_cam, main_frame, side_cams, side_frames, use_farneback=False, want_depth=False, copy=True):
        """mvs_process_frame: recon.cpp:65-117 for one main frame -> (N, 7) points [, depth after mixBackground].
        The library writes into a caller-owned H*W x 7 buffer; this wrapper keeps ONE such buffer per context (a fresh 58 MB
        numpy array per call at 1080p costs more in page faults than the whole GPU pipeline).  copy=True returns an
        independent array; copy=False returns a view of that buffer, valid until the next call -- what a C++ caller reusing
        its cv::Mat gets, and what the timing scripts use."""
        V = len(side_frames)
        cam = _f32(main_cam, (4, 4))
        mf = _u8(main_frame, (self.H, self.W))
        cams = _f32(np.asarray(side_cams, dtype=np.float32).reshape(V, 4, 4)) if V else np.zeros((1, 4, 4), np.float32)
        frames = [_u8(f, (self.H, self.W)) for f in side_frames]
        arr = (_u8p * max(V, 1))(*[_ptr(f, _u8p) for f in frames])
        if getattr(self, "_pf_out", None) is None:
            self._pf_out = np.zeros((self.H * self.W, 7), np.float32)   # zeros: touch every page once, here
        out = self._pf_out
        depth = np.empty((self.H, self.W), np.float32) if want_depth else None
        n = C.c_int(0)
        self._check(self.lib.mvs_process_frame(self.h, _ptr(cam, _fp), _ptr(mf, _u8p), V, _ptr(cams, _fp), arr,
                                               1 if use_farneback else 0, _ptr(out, _fp), C.byref(n),
                                               _ptr(depth, _fp) if want_depth else None))
        pts = out[:n.value].copy() if copy else out[:n.value]
        return (pts, depth) if want_depth else pts

    def process_frame_slots(self, main_cam, main_slot, side_cams, side_slots, use_farneback=False, want_depth=False, copy=True):
        """mvs_process_frame_slots: process_frame() with the frames taken from the frame store (frame_store / frame_upload)."""
        V = len(side_slots)
        cam = _f32(main_cam, (4, 4))
        cams = _f32(np.asarray(side_cams, dtype=np.float32).reshape(V, 4, 4)) if V else np.zeros((1, 4, 4), np.float32)
        slots = np.ascontiguousarray(np.asarray(list(side_slots) if V else [0], dtype=np.int32))
        if getattr(self, "_pf_out", None) is None:
            self._pf_out = np.zeros((self.H * self.W, 7), np.float32)
        out = self._pf_out
        depth = np.empty((self.H, self.W), np.float32) if want_depth else None
        n = C.c_int(0)
        self._check(self.lib.mvs_process_frame_slots(self.h, _ptr(cam, _fp), int(main_slot), V, _ptr(cams, _fp), _ptr(slots, _i32p),
                                                     1 if use_farneback else 0, _ptr(out, _fp), C.byref(n),
                                                     _ptr(depth, _fp) if want_depth else None))
        pts = out[:n.value].copy() if copy else out[:n.value]
        return (pts, depth) if want_depth else pts

    def filter_points(self, points4, alpha):
        """mvs_filter_points -> ascending indices of the points that survive"""
        pts = _f32(points4)
        assert pts.ndim == 2 and pts.shape[1] == 4
        keep = np.empty(max(pts.shape[0], 1), np.int32)
        n = C.c_int(0)
        self._check(self.lib.mvs_filter_points(self.h, _ptr(pts, _fp), pts.shape[0], float(alpha), _ptr(keep, _i32p), C.byref(n)))
        return keep[:n.value].copy()

    def filter_density(self):
        """mvs_filter_density_fetch -> (N,) float32 densities the last successful filter_points ranked its points by (synchronises)"""
        n = self.lib.mvs_filter_density_count(self.h)   # the library's own N; 0: the fetch reports why there is nothing
        dens = np.empty(max(n, 1), np.float32)
        self._check(self.lib.mvs_filter_density_fetch(self.h, _ptr(dens, _fp)))
        return dens[:n]

    def onecall_bands(self):
        """test hook: the row bands the last one-call sweep() of this context was pipelined in (0: the unbanded path)"""
        return self.lib.mvs_test_onecall_bands(self.h)

    def test_rcp(self, exp_bits):
        a, b = C.c_ulonglong(0), C.c_ulonglong(0)
        self._check(self.lib.mvs_test_rcp(self.h, exp_bits, C.byref(a), C.byref(b)))
        return a.value, b.value
