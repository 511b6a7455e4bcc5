"""ctypes binding of libwassgpu.so (the C ABI declared in include/wass_gpu.h).

There is deliberately NO fallback: if the HIP library is missing or a call
fails, an exception is raised.  The CPU oracle under oracle/ is never used
from here.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# WASS_GPU_LIB: another build of the same library (A/B measurements); there is still no fallback of any kind
SO_PATH = os.environ.get("WASS_GPU_LIB") or os.path.join(_HERE, "libwassgpu.so")

WASS_OK = 0
WASS_ERR_INVALID_ARG = -1
WASS_ERR_NO_MEMORY = -3
WASS_ERR_COST_OVERFLOW = -5


class WassError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libwassgpu error {code}: {msg}")
        self.code = code


class SgmParams(C.Structure):
    """wass_sgm_params -- cv::StereoSGBM set-up of wass_stereo.cpp:742-782."""
    _fields_ = [(n, C.c_int) for n in (
        "min_disp", "num_disp", "win", "P1", "P2", "uniq_ratio", "disp12_max_diff", "prefilter_cap",
        "speckle_win", "speckle_range", "ndirs", "disp_offset")] + [("dense_scale", C.c_double)]


class SgmTimings(C.Structure):
    _fields_ = [("prefilter_ms", C.c_float), ("cost_ms", C.c_float), ("aggregate_ms", C.c_float),
                ("select_ms", C.c_float), ("median_ms", C.c_float), ("total_ms", C.c_float),
                ("aggregate_launches", C.c_int), ("cost_overflow", C.c_int), ("vsum_ms", C.c_float)]


class DebugDesc(C.Structure):
    """wass_debug_desc"""
    _fields_ = [("W0", C.c_int), ("H0", C.c_int), ("roi_l", C.c_int * 4), ("roi_r", C.c_int * 4), ("d_left_crop", C.c_void_p),
                ("d_right_crop", C.c_void_p), ("d_disp16", C.c_void_p), ("d_dispf", C.c_void_p), ("num_disp", C.c_int), ("min_disp", C.c_int),
                ("disp_offset", C.c_int), ("disparity_compensation", C.c_double), ("quality", C.c_int)]


class FrameResult(C.Structure):
    """wass_frame_result"""
    _fields_ = [("zgap", C.c_double), ("n_gaps", C.c_uint64), ("component_size", C.c_uint64), ("found", C.c_int),
                ("refine_ok", C.c_int), ("ransac_plane", C.c_double * 4), ("ransac_inliers", C.c_uint64),
                ("plane", C.c_double * 4), ("refine_inliers", C.c_uint64), ("kept_after_ransac_crop", C.c_uint64),
                ("kept_final", C.c_uint64), ("n_points", C.c_uint64), ("xyzc_bytes", C.c_uint64),
                ("sgm_cost_overflow", C.c_int), ("sgm_timeout", C.c_int), ("n_triangulated", C.c_uint64),
                ("n_inliers_out", C.c_uint64), ("stage_ms", C.c_float * 5), ("reserved", C.c_int),
                ("inliers_text_bytes", C.c_uint64), ("inliers_text_unsupported", C.c_uint32), ("reserved2", C.c_uint32)]


class GridSetup(C.Structure):
    """wass_grid_setup"""
    _fields_ = [("R", C.c_double * 9), ("T", C.c_double * 3), ("baseline", C.c_double), ("xmin", C.c_double), ("xmax", C.c_double),
                ("ymin", C.c_double), ("ymax", C.c_double), ("width", C.c_int), ("height", C.c_int)]


class DctOpts(C.Structure):
    """wass_dct_opts"""
    _fields_ = [("nfreqs", C.c_int), ("max_iters", C.c_int), ("tolerance_change", C.c_double), ("regularizer_alpha", C.c_double),
                ("learning_rate", C.c_double), ("seed", C.c_uint64)]


class DctInfo(C.Structure):
    """wass_dct_info"""
    _fields_ = [("steps", C.c_int), ("converged", C.c_int), ("data_loss", C.c_double), ("reg_loss", C.c_double),
                ("fdelta", C.c_double)]


class GridSeqStats(C.Structure):
    """wass_grid_seq_stats"""
    _fields_ = [("zmin", C.c_double), ("zmax", C.c_double), ("zmean", C.c_double), ("n_frames", C.c_int)]


class LinearOpts(C.Structure):
    """wass_linear_opts"""
    _fields_ = [("max_walk_steps", C.c_int), ("accel_w", C.c_int), ("accel_h", C.c_int), ("timing", C.c_int)]


class LinearInfo(C.Structure):
    """wass_linear_info"""
    _fields_ = [("counts", C.c_uint64 * 4), ("n_taken", C.c_uint64), ("hull_vertices", C.c_int), ("hull_candidates", C.c_int),
                ("accel_w", C.c_int), ("accel_h", C.c_int), ("ms_bucket", C.c_float), ("ms_hull", C.c_float), ("ms_walk", C.c_float)]


class Geom(C.Structure):
    """wass_geom"""
    _fields_ = [("K_left", C.c_double * 9), ("K_right", C.c_double * 9), ("R", C.c_double * 9), ("T", C.c_double * 3),
                ("use_custom", C.c_int), ("R1", C.c_double * 9), ("R2", C.c_double * 9), ("P1", C.c_double * 12),
                ("P2", C.c_double * 12), ("HLi", C.c_double * 9), ("HRi", C.c_double * 9),
                ("disparity_compensation", C.c_double), ("dense_scale", C.c_double)]


class TriParams(C.Structure):
    """wass_tri_params"""
    _fields_ = [("min_angle_deg", C.c_double), ("bbox", C.c_double * 4), ("cam_distance", C.c_double)]


class RefineParams(C.Structure):
    """wass_refine_params"""
    _fields_ = [("xmin", C.c_double), ("xmax", C.c_double), ("ymin", C.c_double), ("ymax", C.c_double),
                ("max_distance", C.c_double), ("weight_by_distance", C.c_int), ("central_third_only", C.c_int)]


class PlaneResult(C.Structure):
    """wass_plane_result"""
    _fields_ = [("found", C.c_int), ("ransac_plane", C.c_double * 4), ("ransac_inliers", C.c_uint64),
                ("plane", C.c_double * 4), ("refine_inliers", C.c_uint64), ("kept_after_ransac_crop", C.c_uint64),
                ("kept_final", C.c_uint64)]


class PolParams(C.Structure):
    """wass_pol_params"""
    _fields_ = [("Pcam", C.c_double * 12), ("Kinv", C.c_double * 9), ("origin", C.c_double * 3), ("datascale", C.c_double),
                ("angle_limit", C.c_double), ("batch", C.c_int), ("total_frames", C.c_int)]


class PolOut(C.Structure):
    """wass_pol_out"""
    _fields_ = [(n, C.c_void_p) for n in ("S", "occlusion", "angles", "dolp", "normals", "rays_cam")]


class PolPrepParams(C.Structure):
    """wass_pol_prep_params"""
    _fields_ = [("hdr", C.c_int), ("outputs", C.c_int), ("clahe_clip", C.c_double), ("clahe_tiles", C.c_int), ("reserved", C.c_int)]


class PolPrepOut(C.Structure):
    """wass_pol_prep_out"""
    _fields_ = [(n, C.c_void_p) for n in ("S", "image", "dolp", "aolp", "channels", "image_f32", "aolp_f32")] + [("ranges", C.c_float * 8)]


class KFilterStatsC(C.Structure):
    """wass_kfilter_stats"""
    _fields_ = [("var_in", C.c_double), ("var_out", C.c_double), ("n_nan", C.c_uint64), ("n_empty_cells", C.c_uint64)]


def default_sgm_params(num_disp: int, ndirs: int = 5, min_disp: int = 1, win: int = 13, p1_mult: int = 2,
                       p2_mult: int = 64, disp_offset: int = 0) -> SgmParams:
    """Defaults of SURVEY.md Appendix C (wass_stereo.cpp:742-759)."""
    return SgmParams(min_disp, num_disp, win, p1_mult * win * win, p2_mult * win * win, 1, -1, 60, -70, 16,
                     ndirs, disp_offset, 1.0)


# every symbol include/wass_gpu.h declares: name -> (restype, argtypes)
_vp, _i, _sz = C.c_void_p, C.c_int, C.c_size_t
SYMBOLS = {
    "wass_version": (C.c_char_p, []),
    "wass_ctx_create": (_i, [_i, C.POINTER(_vp)]),
    "wass_ctx_destroy": (None, [_vp]),
    "wass_last_error": (C.c_char_p, [_vp]),
    "wass_ctx_stream": (_vp, [_vp]),
    "wass_ctx_synchronize": (_i, [_vp]),
    "wass_ctx_set_debug": (_i, [_vp, _i]),
    "wass_ctx_set_tail_overlap": (_i, [_vp, _i]),
    "wass_sgm_disparity": (_i, [_vp, _vp, _vp, _i, _i, _sz, C.POINTER(SgmParams), _vp]),
    "wass_sgm_disparity_dev": (_i, [_vp, _vp, _vp, _i, _i, _sz, C.POINTER(SgmParams), _vp]),
    "wass_sgm_last_timings": (_i, [_vp, C.POINTER(SgmTimings)]),
    "wass_sgm_prev_timings": (_i, [_vp, C.POINTER(SgmTimings)]),
    "wass_sgm_call_count": (_i, [_vp, C.POINTER(C.c_uint64)]),
    "wass_sgm_call_timings": (_i, [_vp, C.c_uint64, C.POINTER(SgmTimings)]),
    "wass_sgm_debug_fetch": (_i, [_vp, _vp, _vp, _vp]),
    "wass_sgm_probe_vsum": (_i, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "wass_sgm_selftest": (_i, [_vp, _i, _i, _i, _i, C.POINTER(C.c_uint64)]),
    "wass_device_count": (_i, [C.POINTER(_i)]),
    "wass_ctx_set_kernel_events": (_i, [_vp, _i]),
    "wass_sgm_kernel_times": (_i, [_vp, C.c_char_p, C.c_size_t, C.POINTER(C.c_float), _i, C.POINTER(_i)]),
    "wass_disparity_postprocess": (_i, [_vp, _vp, _i, _i, C.POINTER(SgmParams), _i, _i, _i, _vp]),
    "wass_disparity_postprocess_dev": (_i, [_vp, _vp, _i, _i, C.POINTER(SgmParams), _i, _i, _i, _vp]),
    "wass_triangulate": (_i, [_vp, _vp, _i, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(Geom), _vp, _i, _i, _vp, _vp,
                              C.POINTER(TriParams), C.POINTER(_vp), C.POINTER(C.c_uint64)]),
    "wass_triangulate_dev": (_i, [_vp, _vp, _i, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(Geom), _vp, _i, _i, _vp, _vp,
                                  C.POINTER(TriParams), C.POINTER(_vp), C.POINTER(C.c_uint64)]),
    "wass_mesh_destroy": (None, [_vp]),
    "wass_mesh_size": (_i, [_vp, C.POINTER(_i), C.POINTER(_i)]),
    "wass_mesh_download": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "wass_mesh_upload": (_i, [_vp, _i, _i, _vp, _vp, _vp, C.POINTER(_vp)]),
    "wass_mesh_zgap_percentile": (_i, [_vp, _vp, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "wass_mesh_keep_biggest_component": (_i, [_vp, _vp, C.c_double, C.POINTER(C.c_uint64)]),
    "wass_ransac_sample": (_i, [_i, _i, _i, _vp]),
    "wass_ransac_sample_seeded": (_i, [C.c_uint32, _i, _i, _i, _vp]),
    "wass_mesh_ransac_plane": (_i, [_vp, _vp, _vp, _i, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_uint64),
                                    C.POINTER(_i)]),
    "wass_mesh_crop_plane": (_i, [_vp, _vp, C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_uint64)]),
    "wass_large_gradient_mask": (_i, [_vp, _i, _i, _vp]),
    "wass_mesh_reject_codes": (_i, [_vp, _vp, _vp]),
    "wass_mesh_refine_plane": (_i, [_vp, _vp, C.POINTER(RefineParams), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "wass_mesh_refinement_inliers": (_i, [_vp, _vp, C.POINTER(RefineParams), _i, C.POINTER(C.POINTER(C.c_double)), C.POINTER(C.c_uint64)]),
    "wass_mesh_remove_outliers": (_i, [_vp, _vp, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_uint64),
                                       C.POINTER(C.c_uint64)]),
    "wass_mesh_fit_plane": (_i, [_vp, _vp, _vp, _i, C.c_double, C.POINTER(RefineParams), C.c_double,
                                 C.POINTER(PlaneResult)]),
    "wass_RT_from_plane": (None, [C.POINTER(C.c_double)] * 5),
    "wass_mesh_encode_xyzc": (_i, [_vp, _vp, C.POINTER(C.c_double), C.POINTER(_vp), C.POINTER(_sz)]),
    "wass_mesh_encode_xyzc_to": (_i, [_vp, _vp, C.POINTER(C.c_double), _vp, _sz, C.POINTER(_sz)]),
    "wass_mesh_encode_xyzc_async": (_i, [_vp, _vp, C.POINTER(C.c_double), _vp, _sz, C.POINTER(_sz)]),
    "wass_mesh_finish_frame_async": (_i, [_vp, _vp, C.c_double, _vp, _i, C.c_double, C.POINTER(RefineParams), C.c_double, _vp, _sz]),
    "wass_mesh_finish_frame_async_ex": (_i, [_vp, _vp, C.c_double, _vp, _i, C.c_double, C.POINTER(RefineParams), C.c_double, _vp, _sz,
                                             _vp, _sz, _i, _vp]),
    "wass_mesh_finish_frame_async_ex2": (_i, [_vp, _vp, C.c_double, _vp, _i, C.c_double, C.POINTER(RefineParams), C.c_double, _vp, _sz,
                                              _vp, _sz, _i, _vp, _vp, _sz]),
    "wass_format_g6": (_i, [C.c_double, _vp]),
    "wass_ctx_frame_inliers": (_i, [_vp, _vp, _sz, C.POINTER(C.c_uint64)]),
    "wass_ctx_frame_result": (_i, [_vp, C.POINTER(FrameResult)]),
    "wass_device_alloc": (_i, [_vp, _sz, C.POINTER(_vp)]),
    "wass_device_free": (None, [_vp, _vp]),
    "wass_download": (_i, [_vp, _vp, _vp, _sz]),
    "wass_download_async": (_i, [_vp, _vp, _vp, _sz]),
    "wass_resize_cubic_u8_dev": (_i, [_vp, _vp, _i, _i, _sz, _vp, _i, _i]),
    "wass_jpeg_encode_dev": (_i, [_vp, _vp, _i, _i, _i, _sz, _i, _vp, _sz, C.POINTER(_sz)]),
    "wass_debug_pictures_async": (_i, [_vp, _vp, C.POINTER(DebugDesc), _vp, C.POINTER(_sz * 8), C.POINTER(C.c_uint64)]),
    "wass_debug_picture_size": (_i, [C.POINTER(DebugDesc), _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "wass_debug_pictures_result": (_i, [_vp, C.c_uint64, C.POINTER(_sz * 8)]),
    "wass_pinned_alloc": (_i, [_vp, _sz, C.POINTER(_vp)]),
    "wass_pinned_free": (None, [_vp, _vp]),
    "wass_free": (None, [_vp]),
    "wass_mesh_grid_idw": (_i, [_vp, _vp, C.POINTER(GridSetup), _vp, _vp]),
    "wass_mesh_grid_idw_ex": (_i, [_vp, _vp, C.POINTER(GridSetup), _i, _vp, _vp]),
    "wass_dct_opts_default": (None, [C.POINTER(DctOpts)]),
    "wass_grid_dct": (_i, [_vp, _vp, _i, _i, C.POINTER(DctOpts), _vp, _vp, _vp, _vp, C.POINTER(DctInfo)]),
    "wass_grid_dct_dev": (_i, [_vp, _vp, _i, _i, C.POINTER(DctOpts), _vp, _vp, _vp, _vp, C.POINTER(DctInfo)]),
    "wass_mesh_grid_dct": (_i, [_vp, _vp, C.POINTER(GridSetup), _i, C.POINTER(DctOpts), _vp, _vp, _vp, _vp, _vp, C.POINTER(DctInfo)]),
    "wass_grid_dct_eval": (_i, [_vp, _vp, _i, _i, _i, C.c_double, _vp, _vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "wass_grid_dct_batch": (_i, [_vp, _vp, _i, _i, _i, C.POINTER(DctOpts), _vp, _vp, _vp, _vp, C.POINTER(DctInfo), C.POINTER(_i)]),
    "wass_grid_dct_batch_dev": (_i, [_vp, _vp, _i, _i, _i, C.POINTER(DctOpts), _vp, _vp, _vp, _vp, C.POINTER(DctInfo), C.POINTER(_i)]),
    "wass_mesh_grid_cells_dev": (_i, [_vp, _vp, C.POINTER(GridSetup), _i, _vp]),
    "wass_grid_median_dev": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "wass_grid_seq_create": (_i, [_vp, _i, _i, C.POINTER(_vp)]),
    "wass_grid_seq_push_dev": (_i, [_vp, _vp, _i, _vp]),
    "wass_grid_seq_finish": (_i, [_vp, _i, C.POINTER(GridSeqStats), _vp, _vp, _vp, _vp]),
    "wass_grid_seq_zero_mean_dev": (_i, [_vp, _vp, _i]),
    "wass_grid_seq_destroy": (None, [_vp]),
    "wass_grid_linear_dev": (_i, [_vp, _vp, _vp, _vp, C.c_size_t, C.POINTER(GridSetup), _vp, _vp, C.POINTER(C.c_uint64)]),
    "wass_grid_linear": (_i, [_vp, _vp, _vp, _vp, C.c_size_t, C.POINTER(GridSetup), _vp, _vp, C.POINTER(C.c_uint64)]),
    "wass_mesh_grid_linear": (_i, [_vp, _vp, C.POINTER(GridSetup), _vp, _vp, C.POINTER(C.c_uint64)]),
    "wass_grid_linear_scratch_bytes": (_i, [C.c_size_t, _i, _i, C.POINTER(C.c_size_t)]),
    "wass_grid_linear_dev_ex": (_i, [_vp, _vp, _vp, _vp, C.c_size_t, C.POINTER(GridSetup), C.POINTER(LinearOpts), _vp, _vp,
                                     C.POINTER(LinearInfo)]),
    "wass_mesh_grid_linear_ex": (_i, [_vp, _vp, C.POINTER(GridSetup), C.POINTER(LinearOpts), _vp, _vp, C.POINTER(LinearInfo)]),
    "wass_quantiles_f64_dev": (_i, [_vp, _vp, _sz, C.POINTER(C.c_double), _i, C.POINTER(C.c_double)]),
    "wass_mesh_aligned_z_quantiles": (_i, [_vp, _vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_double), _i,
                                           C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "wass_quantiles_launch_shape": (None, [C.POINTER(_i), C.POINTER(_i)]),
    "wass_spec3d_scratch_bytes": (_i, [_i, _i, _i, C.POINTER(_sz)]),
    "wass_spec3d_create": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, C.POINTER(_vp)]),
    "wass_spec3d_push": (_i, [_vp, _vp, _sz, _sz, C.c_double]),
    "wass_spec3d_push_dev": (_i, [_vp, _vp, _sz, _sz, C.c_double]),
    "wass_spec3d_finish": (_i, [_vp, C.c_double, _vp, C.POINTER(_i), C.POINTER(_i)]),
    "wass_spec3d_finish_dev": (_i, [_vp, C.c_double, _vp, C.POINTER(_i), C.POINTER(_i)]),
    "wass_spec3d_destroy": (None, [_vp]),
    "wass_spec1d_welch": (_i, [_vp, _vp, _i, _i, _i, C.c_double, C.c_double, _vp]),
    "wass_sosfiltfilt_scratch_bytes": (_i, [_i, _i, _i, _i, _i, _i, C.POINTER(_sz), C.POINTER(_i)]),
    "wass_sosfiltfilt": (_i, [_vp, _vp, _sz, _sz, _i, _i, _i, _vp, _i, _vp, _i, _i, _i, _vp, _sz, _sz]),
    "wass_sosfiltfilt_dev": (_i, [_vp, _vp, _sz, _sz, _i, _i, _i, _vp, _i, _vp, _i, _i, _i, _vp, _sz, _sz]),
    "wass_spatial_filter_scratch_bytes": (_i, [_i, _i, _i, C.POINTER(_sz)]),
    "wass_spatial_filter_create": (_i, [_vp, _i, _i, _vp, _i, C.POINTER(_vp)]),
    "wass_spatial_filter_apply": (_i, [_vp, _vp, _sz, _sz, _i, _vp, _sz, _sz]),
    "wass_spatial_filter_apply_dev": (_i, [_vp, _vp, _sz, _sz, _i, _vp, _sz, _sz]),
    "wass_spatial_filter_destroy": (None, [_vp]),
    "wass_kfilter_scratch_bytes": (_i, [_i, _i, _i, C.POINTER(_sz)]),
    "wass_kfilter_create": (_i, [_vp, _i, _i, _i, C.POINTER(_vp)]),
    "wass_kfilter_set_mask": (_i, [_vp, _vp]),
    "wass_kfilter_set_shell": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _i,
                                    C.POINTER(C.c_uint64)]),
    "wass_kfilter_get_mask": (_i, [_vp, _vp]),
    "wass_kfilter_apply": (_i, [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _i, C.POINTER(KFilterStatsC)]),
    "wass_kfilter_apply_dev": (_i, [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _i, C.POINTER(KFilterStatsC)]),
    "wass_kfilter_set_timing": (_i, [_vp, _i]),
    "wass_kfilter_last_timings": (_i, [_vp, C.POINTER(C.c_float * 10)]),
    "wass_kfilter_destroy": (None, [_vp]),
    "wass_visibility_scratch_bytes": (_i, [_i, _i, _i, _i, _i, C.POINTER(_sz), C.POINTER(_i)]),
    "wass_visibility": (_i, [_vp, _vp, _sz, _sz, _i, _i, _i, _vp, _vp, _vp, C.c_double, C.c_double, _i, _vp, _vp, _vp, _vp]),
    "wass_visibility_dev": (_i, [_vp, _vp, _sz, _sz, _i, _i, _i, _vp, _vp, _vp, C.c_double, C.c_double, _i, _vp, _vp, _vp, _vp]),
    "wass_occlusion_rays": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "wass_occlusion_rays_dev": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "wass_lanczos4_table": (_i, [_vp]),
    "wass_remap_lanczos4": (_i, [_vp, _vp, _i, _i, _sz, _vp, _vp, _i, _i, _vp]),
    "wass_remap_lanczos4_dev": (_i, [_vp, _vp, _i, _i, _sz, _vp, _vp, _i, _i, _vp]),
    "wass_radiance_scratch_bytes": (_i, [_i, _i, _i, _i, _i, _i, _i, C.POINTER(_sz), C.POINTER(_i)]),
    "wass_radiance": (_i, [_vp, _vp, _sz, _sz, _i, _i, _vp, _sz, _sz, _i, _i, _i, _vp, _vp, _vp, C.c_double, _i, _vp]),
    "wass_radiance_dev": (_i, [_vp, _vp, _sz, _sz, _i, _i, _vp, _sz, _sz, _i, _i, _i, _vp, _vp, _vp, C.c_double, _i, _vp]),
    "wass_bgimage_scratch_bytes": (_i, [_i, _i, _i, _i, _i, _i, C.POINTER(_sz), C.POINTER(_i)]),
    "wass_bgimage": (_i, [_vp, _vp, _sz, _sz, _i, _i, _i, _i, _i, _vp, _sz, _sz]),
    "wass_bgimage_dev": (_i, [_vp, _vp, _sz, _sz, _i, _i, _i, _i, _i, _vp, _sz, _sz]),
    "wass_radiance_threshold_scratch_bytes": (_i, [_i, _i, _i, _i, _i, C.POINTER(_sz), C.POINTER(_i)]),
    "wass_radiance_range": (_i, [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "wass_radiance_range_dev": (_i, [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "wass_radiance_hist": (_i, [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _i, _i, _i, _i, _vp, _vp, _vp]),
    "wass_radiance_hist_dev": (_i, [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _i, _i, _i, _i, _vp, _vp, _vp]),
    "wass_radiance_mask": (_i, [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _i, _i, _i, _i, _vp, _vp, _vp]),
    "wass_radiance_mask_dev": (_i, [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _i, _i, _i, _i, _vp, _vp, _vp]),
    "wass_pyrup_scratch_bytes": (_i, [_i, _i, _i, _i, _i, _i, _i, C.POINTER(_sz), C.POINTER(_i)]),
    "wass_pyrup_f32": (_i, [_vp, _vp, _sz, _sz, _i, _i, _i, _i, _vp, _sz, _sz]),
    "wass_pyrup_f32_dev": (_i, [_vp, _vp, _sz, _sz, _i, _i, _i, _i, _vp, _sz, _sz]),
    "wass_pyrup_f64": (_i, [_vp, _vp, _sz, _sz, _i, _i, _i, _i, _vp, _sz, _sz]),
    "wass_pyrup_f64_dev": (_i, [_vp, _vp, _sz, _sz, _i, _i, _i, _i, _vp, _sz, _sz]),
    "wass_radiance_up_scratch_bytes": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, C.POINTER(_sz), C.POINTER(_i)]),
    "wass_radiance_up": (_i, [_vp, _vp, _sz, _sz, _i, _i, _vp, _sz, _sz, _i, _i, _i, _vp, _vp, _vp, C.c_double, _i, _i, _vp]),
    "wass_radiance_up_dev": (_i, [_vp, _vp, _sz, _sz, _i, _i, _vp, _sz, _sz, _i, _i, _i, _vp, _vp, _vp, C.c_double, _i, _i, _vp]),
    "wass_bilinear_table_f32": (_i, [_vp]),
    "wass_remap_linear_f32": (_i, [_vp, _vp, _i, _i, _sz, _vp, _vp, _i, _i, _vp]),
    "wass_remap_linear_f32_dev": (_i, [_vp, _vp, _i, _i, _sz, _vp, _vp, _i, _i, _vp]),
    "wass_polarimetric_scratch_bytes": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, C.POINTER(_sz), C.POINTER(_i)]),
    "wass_polarimetric": (_i, [_vp, _vp, _sz, _sz, _sz, _i, _i, _vp, _sz, _sz, _i, _i, _i, _vp, _vp, C.POINTER(PolParams), _vp,
                               C.POINTER(PolOut), _vp, C.POINTER(C.c_uint64)]),
    "wass_polarimetric_dev": (_i, [_vp, _vp, _sz, _sz, _sz, _i, _i, _vp, _sz, _sz, _i, _i, _i, _vp, _vp, C.POINTER(PolParams), _vp,
                                   C.POINTER(PolOut), _vp, C.POINTER(C.c_uint64)]),
    "wass_clip_cube": (_i, [_vp, _vp, _sz, _sz, _i, _i, _i, C.c_float, C.c_float, _vp, _sz, _sz, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "wass_clip_cube_dev": (_i, [_vp, _vp, _sz, _sz, _i, _i, _i, C.c_float, C.c_float, _vp, _sz, _sz, C.POINTER(C.c_float),
                                C.POINTER(C.c_float)]),
    "wass_zeromean": (_i, [_vp, _vp, _sz, _sz, _i, _i, _i, _vp, _sz, _sz]),
    "wass_zeromean_dev": (_i, [_vp, _vp, _sz, _sz, _i, _i, _i, _vp, _sz, _sz]),
    "wass_wavestats_scratch_bytes": (_i, [_i, _i, _i, C.c_double, C.c_double, _i, _i, C.c_double, _i, _i, C.POINTER(_sz), C.POINTER(_i)]),
    "wass_wavestats": (_i, [_vp, _vp, _sz, _sz, _i, _i, _i, C.c_double, C.c_double, _i, _i, _i, C.c_double, _i, _vp, _vp, _vp]),
    "wass_wavestats_dev": (_i, [_vp, _vp, _sz, _sz, _i, _i, _i, C.c_double, C.c_double, _i, _i, _i, C.c_double, _i, _vp, _vp, _vp]),
    "wass_specprod_scratch_bytes": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, C.POINTER(_sz), C.POINTER(_i)]),
    "wass_specprod_tables": (_i, [_vp, _vp, _i, _i, _i, _i, C.c_double, _vp, _i, _vp, _i, _i, _vp, _vp, _vp, C.POINTER(C.c_double),
                                  C.POINTER(C.c_int64)]),
    "wass_specprod_tables_dev": (_i, [_vp, _vp, _i, _i, _i, _i, C.c_double, _vp, _i, _vp, _i, _vp, _vp, _vp, C.POINTER(C.c_double),
                                      C.POINTER(C.c_int64)]),
    "wass_specprod_peak_dev": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, C.c_double, _vp, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "wass_specprod_current_sums_dev": (_i, [_vp, _vp, _i, _i, _i, _i, _i, C.c_double, _vp, _vp, _vp, _vp, _vp, C.c_double, C.c_double,
                                            C.c_double, C.c_double, _vp, C.POINTER(C.c_int64)]),
    "wass_match_scratch_bytes": (_i, [_i, _i, C.POINTER(_sz)]),
    "wass_match_knn": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _vp, _vp]),
    "wass_match_knn_dev": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _vp, _vp]),
    "wass_match_payoff": (_i, [_vp, _vp, _i, _vp, _i, _vp, _i, C.c_double, _vp]),
    "wass_match_payoff_dev": (_i, [_vp, _vp, _sz, _vp, _sz, _vp, _sz, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), _i, C.c_double, _vp, _sz]),
    "wass_match_iidyn": (_i, [_vp, _vp, _i, _vp, _i, C.c_double, _i, C.c_double, C.POINTER(_i), C.POINTER(C.c_double), _vp, C.POINTER(_i)]),
    "wass_match_iidyn_dev": (_i, [_vp, _vp, _sz, _vp, _sz, _i, C.POINTER(_i), _i, C.c_double, _i, C.c_double, C.POINTER(_i),
                                  C.POINTER(C.c_double), _vp, _sz, C.POINTER(_i)]),
    "wass_match_round_dev": (_i, [_vp, _vp, _sz, _vp, _sz, _vp, _sz, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), _i, C.c_double, C.c_double, _i,
                                  C.c_double, _vp, _sz, _vp, _sz, C.POINTER(_i), C.POINTER(C.c_double), _vp, _sz, C.POINTER(_i)]),
    "wass_epi_scratch_bytes": (_i, [_i, _i, C.POINTER(_sz)]),
    "wass_epi_solve5_dev": (_i, [_vp, _vp, _vp, _sz, _vp, _sz, C.POINTER(_i), _i, _i, _vp, _vp]),
    "wass_epi_score_dev": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _sz, C.POINTER(_i), C.POINTER(C.c_double), _i, _vp]),
    "wass_epi_mask_dev": (_i, [_vp, _vp, _vp, _vp, _sz, C.POINTER(_i), C.POINTER(C.c_double), _i, _vp, _vp, _sz]),
    "wass_epi_find_dev": (_i, [_vp, _vp, _vp, _sz, _vp, _sz, C.POINTER(_i), C.POINTER(C.c_double), _i, _i, _vp, C.POINTER(_i), C.POINTER(_i),
                               _vp, _vp, _sz]),
    "wass_ac_scratch_bytes": (_i, [_i, C.POINTER(_sz)]),
    "wass_ac_triangulate_dev": (_i, [_vp, _vp, _vp, _vp, _i, C.POINTER(C.c_double), C.POINTER(C.c_double), _vp, C.POINTER(C.c_int32)]),
    "wass_ac_linearize_dev": (_i, [_vp, C.POINTER(C.c_double), _vp, _vp, _i, _vp, C.POINTER(C.c_double)]),
    "wass_ac_step_dev": (_i, [_vp, C.POINTER(C.c_double), _vp, _vp, _i, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), _vp, _vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(_i)]),
    "wass_ac_error_dev": (_i, [_vp, C.POINTER(C.c_double), _vp, _vp, _i, _vp, C.POINTER(C.c_double)]),
    "wass_ac_bundle_dev": (_i, [_vp, C.POINTER(C.c_double), _vp, _vp, _i, _i, C.POINTER(C.c_double)]),
    "wass_kaze_scratch_bytes": (_i, [_i, _i, _i, C.POINTER(_sz)]),
    "wass_kaze_convert_dev": (_i, [_vp, _vp, _sz, _i, _i, C.c_float, _vp]),
    "wass_kaze_gauss_dev": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _vp]),
    "wass_kaze_scharr_dev": (_i, [_vp, _vp, _i, _i, _i, C.c_float, C.c_float, _vp, _vp]),
    "wass_kaze_hessian_dev": (_i, [_vp, _vp, _vp, _i, _i, _i, C.c_float, C.c_float, _vp, _vp, _vp, _vp]),
    "wass_kaze_contrast_dev": (_i, [_vp, _vp, _vp, _i, _i, _vp, C.POINTER(C.c_float), C.POINTER(C.c_uint32), _vp]),
    "wass_kaze_flow_dev": (_i, [_vp, _vp, _vp, _i, _i, C.c_float, _vp]),
    "wass_kaze_diffuse_dev": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _i]),
    "wass_kaze_extrema_dev": (_i, [_vp, _vp, _sz, _i, _i, _i, C.c_float, _vp, _vp, _i, _vp, C.POINTER(C.c_uint32)]),
    "wass_kaze_refine_dev": (_i, [_vp, _vp, _sz, _i, _i, _i, _vp, _i, _vp]),
    "wass_kaze_orientation_dev": (_i, [_vp, _vp, _i, _vp, _vp, _sz, _i, _i, _i, _vp]),
    "wass_kaze_descriptors_dev": (_i, [_vp, _vp, _i, _vp, _vp, _sz, _i, _i, _i, _vp]),
    "wass_vref_scratch_bytes": (_i, [_i, _i, _i, _i, _i, _i, C.POINTER(_sz)]),
    "wass_vref_create": (_i, [_vp, _i, _i, _vp, _vp, _vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                              C.POINTER(C.c_double), _vp, _i, _i, _vp, _i, _i, _vp, C.POINTER(_vp)]),
    "wass_vref_destroy": (None, [_vp]),
    "wass_vref_sample": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "wass_vref_zgrad": (_i, [_vp, _vp, _vp, _vp]),
    "wass_vref_loss": (_i, [_vp, _vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "wass_vref_gradient": (_i, [_vp, _vp, C.c_double, _vp, _vp]),
    "wass_vref_adjoint": (_i, [_vp, _vp, _vp, _vp, C.c_double, _vp, _vp]),
    "wass_vref_optimize": (_i, [_vp, _vp, _vp, _vp, C.POINTER(C.c_int64), _i, C.c_double, C.c_double, C.c_double, _i, _vp, _i,
                                C.POINTER(_i), _vp]),
    "wass_vref_batch_scratch_bytes": (_i, [_i, _i, _i, _i, _i, _i, _i, C.POINTER(_sz)]),
    "wass_vref_batch_create": (_i, [_vp, _i, _i, _i, _vp, _vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                    C.POINTER(C.c_double), _i, _i, _i, _i, _vp, C.POINTER(_vp)]),
    "wass_vref_batch_destroy": (None, [_vp]),
    "wass_vref_batch_load": (_i, [_vp, _i, _vp, _vp, _vp, _vp, C.c_double]),
    "wass_vref_batch_set_state": (_i, [_vp, _vp, _vp, _vp, C.c_int64]),
    "wass_vref_batch_get_state": (_i, [_vp, _vp, _vp, _vp, C.POINTER(C.c_int64)]),
    "wass_vref_batch_optimize": (_i, [_vp, _i, C.c_double, C.c_double, C.c_double, _i, _vp, _i, C.POINTER(_i)]),
    "wass_vref_batch_result": (_i, [_vp, _vp, _vp]),
    "wass_planes_mean_accumulate": (None, [C.POINTER(C.c_double), _i, C.POINTER(C.c_double)]),
    "wass_planes_mean_finish": (None, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(_i)]),
    "wass_ctx_wait_for_stream": (_i, [_vp, _vp]),
    "wass_dense_input_size": (_i, [_i, _i, C.c_double, C.POINTER(_i), C.POINTER(_i)]),
    "wass_disparity_postprocess_ex": (_i, [_vp, _vp, _i, _i, C.POINTER(SgmParams), _i, _i, _i, _i, _i, _i, _vp]),
    "wass_disparity_postprocess_ex_dev": (_i, [_vp, _vp, _i, _i, C.POINTER(SgmParams), _i, _i, _i, _i, _i, _i, _vp]),
    "wass_biggest_component_by_gradient_dev": (_i, [_vp, _vp, _i, _i, _i]),
    "wass_filter_speckles_dev": (_i, [_vp, _vp, _i, _i, _i, _i, _i]),
    "wass_upload_async": (_i, [_vp, _vp, _vp, _sz]),
    "wass_burned_area_mask_dev": (_i, [_vp, _vp, _sz, _vp]),
    "wass_camera_mask_dev": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "wass_clahe": (_i, [_vp, _vp, _i, _i, _sz, C.c_double, _i, _i, _vp]),
    "wass_clahe_dev": (_i, [_vp, _vp, _i, _i, _sz, C.c_double, _i, _i, _vp]),
    "wass_coll_unique_id": (_i, [_vp]),
    "wass_coll_init": (_i, [_vp, _i, _i, _vp]),
    "wass_coll_allreduce_sum_f64": (_i, [_vp, C.POINTER(C.c_double), _i]),
    "wass_stereo_rectify": (_i, [C.POINTER(C.c_double), C.POINTER(C.c_double), _i, _i, C.POINTER(C.c_double),
                                 C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                 C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(_i), C.POINTER(_i)]),
    "wass_init_rectify_map": (_i, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), _i, _i, _vp, _vp]),
    "wass_remap_cubic": (_i, [_vp, _vp, _i, _i, _sz, _vp, _vp, _i, _i, C.POINTER(_i), _vp]),
    "wass_remap_cubic_dev": (_i, [_vp, _vp, _i, _i, _sz, _vp, _vp, _i, _i, C.POINTER(_i), _vp]),
    "wass_undistort": (_i, [_vp, _vp, _i, _i, _sz, C.POINTER(C.c_double), C.POINTER(C.c_double), _i, _vp]),
    "wass_undistort_dev": (_i, [_vp, _vp, _i, _i, _sz, C.POINTER(C.c_double), C.POINTER(C.c_double), _i, _vp]),
    "wass_prepare_pol": (_i, [_vp, _vp, _i, _i, _sz, C.POINTER(C.c_double), C.POINTER(C.c_double), _i, C.POINTER(PolPrepParams),
                              C.POINTER(PolPrepOut)]),
    "wass_prepare_pol_dev": (_i, [_vp, _vp, _i, _i, _sz, C.POINTER(C.c_double), C.POINTER(C.c_double), _i, C.POINTER(PolPrepParams),
                                  C.POINTER(PolPrepOut)]),
    "wass_warp_perspective": (_i, [_vp, _vp, _i, _i, _sz, C.POINTER(C.c_double), _i, _i, C.POINTER(_i), _vp]),
    "wass_warp_perspective_dev": (_i, [_vp, _vp, _i, _i, _sz, C.POINTER(C.c_double), _i, _i, C.POINTER(_i), _vp]),
}

_lib = None


def load() -> C.CDLL:
    """Load libwassgpu.so and bind every declared symbol; raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise ImportError(
            f"{SO_PATH} not found: build the HIP extension first (python -m wass_amd.build). "
            "wass_amd has no CPU fallback.")
    # PyTorch bundles its own libamdhip64 (NEEDED as the unversioned "libamdhip64.so", SONAME .so.7).
    # If /opt/rocm's copy were loaded first, a later `import torch` would pull in a SECOND HIP runtime
    # and fail with "No HIP GPUs are available"; importing torch first makes both share one runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(SO_PATH)
    other_build = bool(os.environ.get("WASS_GPU_LIB"))
    for name, (res, args) in SYMBOLS.items():
        if other_build and not hasattr(lib, name):
            continue                     # an OLDER build of the library in an A/B measurement: newer entry points are simply absent
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def scratch_bytes(name: str, args, refusal: str) -> int:
    """What the pure planner wass_<name>_scratch_bytes(*args, &bytes) answers (no GPU needed); where it refuses, a ValueError with
    the caller's text."""
    b = C.c_size_t()
    if getattr(load(), f"wass_{name}_scratch_bytes")(*args, C.byref(b)) != 0:
        raise ValueError(refusal)
    return b.value
