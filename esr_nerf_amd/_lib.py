"""ctypes binding of libesr_hip.so (include/esr_hip.h).

The library is the product: if it is missing or fails to load, everything that
needs it raises -- there is no CPU or PyTorch fallback on the product path.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libesr_hip.so")
# developer experiments only (python -m esr_nerf_amd.build --variant builds alternative libraries; tools/ab_env.sh times them
# side by side on one box)
LIB_PATH = os.environ.get("ESR_LIB_PATH", LIB_PATH)
ABI_VERSION = 43
_lib = None


class EsrScene(C.Structure):
    _fields_ = [
        ("xyz_min", C.c_float * 3), ("xyz_max", C.c_float * 3),
        ("mask_min", C.c_float * 3), ("mask_max", C.c_float * 3),
        ("gx", C.c_int32), ("gy", C.c_int32), ("gz", C.c_int32),
        ("mx", C.c_int32), ("my", C.c_int32), ("mz", C.c_int32),
        ("near_", C.c_float), ("stepdist", C.c_float), ("voxel_size", C.c_float),
        ("act_shift", C.c_float), ("mask_thres", C.c_float), ("fast_thres", C.c_float),
        ("s_val", C.c_float), ("max_steps", C.c_int32), ("grad_feat", C.c_float * 4),
    ]


class EsrPlan(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ("n_on", "n_off", "tiles_on", "tiles_all", "m0", "m1", "m2", "overflow")]


class EsrMarch(C.Structure):               # esr_march_t
    _fields_ = [("scene", C.POINTER(EsrScene))] + \
               [(n, C.c_void_p) for n in ("rays_o", "rays_d", "viewdirs", "mask_density", "sdf", "gg")] + \
               [("n_rays", C.c_int32), ("flags", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("cnt3", "alphainv_last", "cum_weights", "ray_stats", "plan", "off3", "rec_ray",
                                          "rec_step", "rec_w", "rec_sdf", "dweight", "dlast", "grad_sdf", "grad_gg",
                                          "dsdf_rec")] + \
               [("accumulate", C.c_int32), ("cache", C.c_void_p)]


MARCH_COARSE, MARCH_GRAD_ALPHA = 1, 2      # ESR_MARCH_COARSE, ESR_MARCH_GRAD_ALPHA


class EsrFeatArgs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("rays_o", "rays_d", "viewdirs", "rec_ray", "rec_step", "rec_sdf",
                                          "pts", "pt_viewdirs", "pt_sdf")] + \
               [("n_pts", C.c_int32), ("sdf", C.c_void_p), ("color_on", C.c_void_p * 3),
                ("color_off", C.c_void_p * 3), ("tiles_on", C.c_int32), ("tiles_all", C.c_int32)]


class EsrFeatBwdSrc(C.Structure):
    _fields_ = [("dX", C.c_void_p), ("grad_color_on", C.c_void_p), ("grad_color_off", C.c_void_p),
                ("t0", C.c_int32), ("t1", C.c_int32)]


class EsrLtsArgs(C.Structure):
    _fields_ = [("n_pts", C.c_int32), ("n_rays", C.c_int32), ("n_sg", C.c_int32), ("pdra_mode", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("base", "rough", "metal", "normal", "view", "dirs", "off_m", "emo_m",
                                          "last2", "mus", "lambdas", "lobes", "emission", "umask")]


class EsrLtsGather(C.Structure):          # esr_lts_gather_t
    _fields_ = [(n, C.c_void_p) for n in ("jp", "ray64", "pts_all", "eg", "rec_sdf", "viewdirs", "brdf_a", "emit_a",
                                          "umask_rays")] + [("n_pts", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("pts2", "vd2", "sdf2", "normal", "base", "rough", "metal", "emis", "umask", "pt1")]


class EsrActJob(C.Structure):             # esr_act_job_t
    _fields_ = [("z", C.c_void_p), ("g_tile", C.c_void_p), ("out", C.c_void_p), ("tiles", C.c_int32), ("rows", C.c_int32),
                ("n_ch", C.c_int32), ("act", C.c_int32), ("bwd", C.c_int32), ("src", C.c_void_p), ("src_c", C.c_int32),
                ("n_src", C.c_int32), ("inv", C.c_void_p), ("pt1", C.c_void_p), ("ex", C.c_void_p * 3),
                ("ex_c", C.c_int32 * 3), ("ex_col0", C.c_int32 * 3)]


class EsrGatherJob(C.Structure):          # esr_gather_job_t
    _fields_ = [("src", C.c_void_p), ("tile_rows", C.c_int32), ("row_stride", C.c_int32), ("col0", C.c_int32),
                ("n_ch", C.c_int32), ("perm", C.c_void_p), ("n", C.c_int32), ("out", C.c_void_p)]


class EsrPairJob(C.Structure):            # esr_pair_job_t
    _fields_ = [("a", C.c_void_p), ("b", C.c_void_p), ("rows", C.c_int64), ("cols", C.c_int32), ("row_mask", C.c_void_p),
                ("mask_value", C.c_int32), ("count_dev", C.c_void_p), ("kind", C.c_int32), ("w_value", C.c_float),
                ("w_a", C.c_float), ("w_b", C.c_float), ("ga", C.c_void_p), ("gb", C.c_void_p)]


class EsrLtsGrads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("d_off_m", "d_emo_m", "d_last2", "d_base", "d_rough", "d_metal",
                                          "d_emission", "d_mus", "d_lambdas", "d_lobes")]


class EsrCdIndex(C.Structure):           # esr_cd_index_t
    _fields_ = [("origin", C.c_double * 3), ("h", C.c_double), ("dims", C.c_int32 * 3), ("coarse", C.c_int32),
                ("cap", C.c_int64), ("keys", C.c_void_p), ("cells", C.c_void_p), ("start", C.c_void_p), ("pts", C.c_void_p),
                ("ids", C.c_void_p), ("ccap", C.c_int64), ("ckeys", C.c_void_p)]


class EsrDvgo(C.Structure):             # esr_dvgo_t
    _fields_ = [("density", C.c_void_p), ("off_color", C.c_void_p), ("emo_color", C.c_void_p), ("dims", C.c_int32 * 3),
                ("xyz_min", C.c_float * 3), ("xyz_max", C.c_float * 3)] + \
               [(n, C.c_float) for n in ("near_", "far_", "step_scale", "interval", "act_shift")] + [("n_samples", C.c_int32)]


class EsrDvgoRays(C.Structure):         # esr_dvgo_rays_t
    _fields_ = [(n, C.c_void_p) for n in ("rays_o", "rays_d", "nrm", "jitter", "em_modes")] + \
               [("em_all", C.c_int32), ("n_rays", C.c_int64)]


class EsrDvgoOut(C.Structure):          # esr_dvgo_out_t
    _fields_ = [(n, C.c_void_p) for n in ("alpha", "alphainv_cum", "weights", "raw_rgb", "rgb", "depth", "disp", "white_bg",
                                          "off_rgb", "on_rgb", "emo_rgb")]


class EsrDvgoBwd(C.Structure):          # esr_dvgo_bwd_t
    _fields_ = [(n, C.c_void_p) for n in ("alpha", "alphainv_cum", "raw_rgb", "g_alphainv_cum", "g_weights", "g_raw_rgb",
                                          "g_rgb", "grad_density", "grad_off", "grad_emo")]


class EsrViewPost(C.Structure):         # esr_view_post_t
    _fields_ = [("v", C.c_void_p), ("wbg", C.c_void_p), ("wbg_scale", C.c_float), ("lin", C.c_int32), ("n", C.c_int64),
                ("channels", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("out", "gamma", "out_u8", "gamma_u8", "target_out", "target_gamma", "partials",
                                          "sqerr")]


class EsrCamera(C.Structure):           # esr_camera_t
    _fields_ = [(n, C.c_float) for n in ("fx", "fy", "cx", "cy")] + [(n, C.c_int32) for n in ("width", "height", "n_views")]


CAMERA_LDS_VIEWS = 256                  # ESR_CAMERA_LDS_VIEWS
CAMERA_BOUNDS_BLOCKS = 1024             # ESR_CAMERA_BOUNDS_BLOCKS
RESAMPLE_MAX_C = 16                     # ESR_RESAMPLE_MAX_C
DENSITY_BOUNDS_BLOCKS = 1024            # ESR_DENSITY_BOUNDS_BLOCKS
PARTITION_BLOCK = 1024                  # ESR_PARTITION_BLOCK
PARTITION_SCAN_TILE = 1024              # ESR_PARTITION_SCAN_TILE
SIMPLIFY_MAX_C = 16                     # ESR_SIMPLIFY_MAX_C
SIMPLIFY_DEBUG = 15                     # ESR_SIMPLIFY_DEBUG


class EsrRegroupStats(C.Structure):     # esr_regroup_stats_t
    _fields_ = [(n, C.c_int64) for n in ("n_set", "n_clear", "n_nan")] + \
               [(n, C.c_float) for n in ("min_all", "max_all", "min_set", "max_set", "min_clear", "max_clear")]


class EsrMlpWeights(C.Structure):
    _fields_ = [("w", C.c_void_p * 4), ("b", C.c_void_p * 4)]


class EsrWgradJob(C.Structure):
    """esr_wgrad_job_t"""
    _fields_ = [("kind", C.c_int32), ("color_row0", C.c_int32), ("t0", C.c_int32), ("t1", C.c_int32),
                ("X", C.c_void_p), ("H", C.c_void_p), ("dZ", C.c_void_p), ("dz", C.c_void_p),
                ("gw", C.c_void_p), ("gb", C.c_void_p), ("X16", C.c_void_p), ("amax", C.c_void_p)]


# every exported symbol of include/esr_hip.h (checked by tests/test_host.py::test_library_loads_and_exports_every_header_symbol)
EXPORTS = [
    "esr_abi_version", "esr_build_info",
    "esr_sample_count", "esr_sample_fill", "esr_alpha2weight_fwd", "esr_alpha2weight_bwd",
    "esr_tv_add_grad", "esr_segment_sum",
    "esr_sample_count_f64", "esr_sample_fill_f64", "esr_alpha2weight_fwd_f64", "esr_alpha2weight_bwd_f64",
    "esr_infer_t_minmax", "esr_infer_n_samples", "esr_infer_ray_start_dir", "esr_sample_ndc_pts", "esr_sample_bg_pts",
    "esr_maskcache_lookup", "esr_raw2alpha", "esr_raw2alpha_bwd", "esr_tv_add_grad_masked",
    "esr_march_count", "esr_march_fill", "esr_march_bwd", "esr_fine_march_cache_floats",
    "esr_fine_plan_begin", "esr_fine_plan", "esr_fine_plan_totals", "esr_fine_plan_offsets",
    "esr_fine_feat_fwd", "esr_fine_feat_fwd_x16", "esr_fine_feat_x16_bytes", "esr_fine_feat_bwd",
    "esr_mlp_packed_floats", "esr_mlp_pack", "esr_mlp_pack_batch", "esr_mlp_packed_split_elems", "esr_mlp_split_gain_offset", "esr_mlp_split_range_flag", "esr_mlp_fwd_split", "esr_mlp_fwd_fine_split", "esr_mlp_dgrad_split", "esr_mlp_dgrad_fine_split", "esr_absmax", "esr_mlp_fwd", "esr_mlp_fwd_mixed", "esr_mlp_fwd_fine", "esr_mlp_dgrad_fine", "esr_mlp_fwd_fine_bf16", "esr_mlp_dgrad_fine_bf16", "esr_mlp_dgrad", "esr_mlp_wgrad", "esr_mlp_wgrad_batch", "esr_tone_wgrad_scratch_floats", "esr_tone_wgrad_recompute", "esr_tone_wgrad_recompute_bf16", "esr_tone_wgrad_recompute_split",
    "esr_mlp_wgrad_scratch_floats",
    "esr_fine_tone_in_fwd", "esr_fine_composite_fwd", "esr_fine_composite_bwd",
    "esr_fine_tone_in_bwd", "esr_fine_tone_dgrad_split", "esr_fine_loss_fwd_bwd_dp",
    "esr_expgrad_fwd", "esr_expgrad_bwd", "esr_lts_dirs", "esr_lts_ref_order", "esr_lts_perturb", "esr_lts_gather_rows",
    "esr_lts_gather_points", "esr_lts_combine_fwd", "esr_lts_combine_bwd",
    "esr_act_fwd", "esr_act_bwd", "esr_act_batch", "esr_lts_gather_rows_batch", "esr_pair_loss_batch", "esr_lts_ref_order_inv", "esr_lts_dirs_rays", "esr_composite3_fwd", "esr_composite3_bwd", "esr_lts_tone_in_bwd",
    "esr_sample_points", "esr_pair_loss_fwd_bwd", "esr_emit_edit",
    "esr_gauss3d_fwd", "esr_gauss3d_bwd", "esr_central_grad_fwd", "esr_central_grad_bwd",
    "esr_coarse_feat_fwd", "esr_coarse_feat_bwd", "esr_coarse_shade_fwd", "esr_coarse_shade_bwd",
    "esr_adam_step", "esr_eval_aux", "esr_eval_disp",
    "esr_mlp_packed_bf16_elems", "esr_mlp_pack_bf16", "esr_mlp_fwd_bf16", "esr_mlp_dgrad_bf16", "esr_mlp_wgrad_bf16",
    "esr_brick_floats", "esr_brick_flags", "esr_brick_pack", "esr_brick_unpack", "esr_brick_list", "esr_brick_list_scratch_ints",
    "esr_smooth_grad_tv_fwd", "esr_smooth_grad_tv_bwd", "esr_host_choice_noreplace", "esr_host_choice_start", "esr_host_choice_wait",
    "esr_mesh_field", "esr_mesh_blocks", "esr_mesh_count", "esr_mesh_emit",
    "esr_cd_sample_count", "esr_cd_sample_fill", "esr_cd_cell_keys", "esr_cd_hash_insert", "esr_cd_downsample_round",
    "esr_cd_nn",
    "esr_dvgo_fwd", "esr_dvgo_eval", "esr_dvgo_bwd", "esr_dvgo_count", "esr_dvgo_count_add",
    "esr_ssim", "esr_view_post", "esr_sqerr_sum", "esr_gamma_curve", "esr_mask_iou",
    "esr_mask_dilate", "esr_edit_label",
    "esr_ray_filter",
    "esr_adam_step_live", "esr_brick_live_from_moments",
    "esr_camera_rays", "esr_camera_batch", "esr_camera_bounds", "esr_ray_filter_cameras",
    "esr_grid_resample", "esr_maxpool3d", "esr_nonempty_mask", "esr_density_bounds",
    "esr_cc_link", "esr_cc_flatten", "esr_cc_face_labels", "esr_cc_stats",
    "esr_emit_decide", "esr_emit_decide_bits", "esr_flags_pack", "esr_flags_unpack", "esr_flag_scan_bits",
    "esr_index_partition_bits", "esr_regroup_stats_merge",
    "esr_conv_packed_floats", "esr_conv_pack", "esr_conv_relu", "esr_maxpool_nhwc", "esr_lpips_layer",
    "esr_raster_faces", "esr_raster_resolve", "esr_source_masks",
    "esr_simplify_cell_keys", "esr_simplify_pair_keys", "esr_simplify_clusters", "esr_simplify_face_keys", "esr_simplify_keep",
    "esr_bvh_keys", "esr_bvh_tree", "esr_bvh_fit", "esr_bvh_cast",
]

# full ctypes signatures (argument conversion checked on every call) of the entries that declare them
SIGNATURES = {
    **{f"esr_march_{w}": (C.c_int, [C.POINTER(EsrMarch), C.c_void_p]) for w in ("count", "fill", "bwd")},
    "esr_mask_dilate": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "esr_edit_label": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_float, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p]),
    "esr_ray_filter": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_int32,
                                 C.c_void_p, C.c_void_p, C.c_void_p]),
    "esr_adam_step_live": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                     C.c_float, C.c_float, C.c_float, C.c_float, C.c_int32, C.c_int32, C.c_void_p,
                                     C.c_void_p]),
    "esr_brick_live_from_moments": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "esr_camera_rays": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p]),
    "esr_camera_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_float,
                                   C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p]),
    "esr_camera_bounds": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "esr_ray_filter_cameras": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_int32,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "esr_grid_resample": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                    C.c_int32, C.c_void_p]),
    "esr_maxpool3d": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "esr_nonempty_mask": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.c_float, C.c_float,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    "esr_density_bounds": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.c_float, C.c_float,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "esr_cc_link": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "esr_cc_flatten": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "esr_cc_face_labels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "esr_cc_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_int32,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p]),
    "esr_emit_decide": (C.c_int, [C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "esr_emit_decide_bits": (C.c_int, [C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "esr_flags_pack": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "esr_flags_unpack": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "esr_flag_scan_bits": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "esr_index_partition_bits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "esr_regroup_stats_merge": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "esr_conv_packed_floats": (C.c_int64, [C.c_int32] * 4),
    "esr_conv_pack": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "esr_conv_relu": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "esr_maxpool_nhwc": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                   C.c_void_p]),
    "esr_lpips_layer": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p]),
    "esr_raster_faces": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                   C.c_double, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                   C.c_void_p]),
    "esr_raster_resolve": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "esr_source_masks": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32,
                                   C.c_void_p, C.c_void_p, C.c_void_p]),
    "esr_simplify_cell_keys": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]),
    "esr_simplify_pair_keys": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "esr_simplify_clusters": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_double,
                                        C.c_double, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "esr_simplify_face_keys": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "esr_simplify_keep": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                    C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "esr_bvh_keys": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "esr_bvh_tree": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "esr_bvh_fit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "esr_bvh_cast": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                               C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}


def lib() -> C.CDLL:
    """Load the HIP library; raises (never falls back) when it is unavailable."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -m esr_nerf_amd.build` "
                "(there is no CPU fallback for the HIP path)")
        L = C.CDLL(LIB_PATH)
        L.esr_abi_version.restype = C.c_int
        L.esr_build_info.restype = C.c_char_p
        if hasattr(L, "esr_mlp_packed_floats"):
            L.esr_mlp_packed_floats.restype = C.c_int64
            L.esr_mlp_wgrad_scratch_floats.restype = C.c_int64
            L.esr_tone_wgrad_scratch_floats.restype = C.c_int64
            L.esr_fine_march_cache_floats.restype = C.c_int64
        if hasattr(L, "esr_fine_feat_x16_bytes"):
            L.esr_fine_feat_x16_bytes.restype = C.c_int64
        if hasattr(L, "esr_brick_list_scratch_ints"):
            L.esr_brick_list_scratch_ints.restype = C.c_int64
        if hasattr(L, "esr_mlp_packed_bf16_elems"):
            L.esr_mlp_packed_bf16_elems.restype = C.c_int64
        if hasattr(L, "esr_mlp_packed_split_elems"):
            L.esr_mlp_packed_split_elems.restype = C.c_int64
        if hasattr(L, "esr_mlp_split_gain_offset"):
            L.esr_mlp_split_gain_offset.restype = C.c_int64
        if hasattr(L, "esr_mesh_blocks"):
            L.esr_mesh_blocks.restype = C.c_int64
        for name in ("esr_cd_sample_count", "esr_cd_sample_fill", "esr_cd_cell_keys", "esr_cd_hash_insert",
                     "esr_cd_downsample_round", "esr_cd_nn", "esr_ssim", "esr_view_post", "esr_sqerr_sum", "esr_gamma_curve",
                     "esr_mask_iou"):
            if hasattr(L, name):
                getattr(L, name).restype = C.c_int
        for name, (res, args) in SIGNATURES.items():
            if hasattr(L, name):
                getattr(L, name).restype, getattr(L, name).argtypes = res, args
        if L.esr_abi_version() != ABI_VERSION:
            raise RuntimeError("libesr_hip.so ABI version mismatch: rebuild")
        _lib = L
    return _lib


def check(code: int, what: str):
    if code != 0:
        raise RuntimeError(f"{what} failed with code {code}" +
                           (" (hipError)" if code > 0 else
                            " (a capacity limit of the kernels is exceeded, include/esr_hip.h: ESR_ECAP)" if code == -2 else
                            " (bad argument)"))


def ptr(t):
    """Device pointer of a contiguous CUDA(HIP) tensor (or NULL for None)."""
    if t is None:
        return C.c_void_p(0)
    if not t.is_cuda:
        raise RuntimeError("esr_hip ops need device tensors (got a CPU tensor)")
    if not t.is_contiguous():
        raise RuntimeError("esr_hip ops need contiguous tensors")
    return C.c_void_p(t.data_ptr())


_dev_index = {}


def stream_ptr(device=None):
    """The current HIP stream of ``device`` as a void pointer.  (``torch.cuda.current_stream(device).cuda_stream`` builds a
    Stream object per call, ~5 us; a light-transport step asks ~100 times -- the raw getter is what torch's own
    compiled code uses.)"""
    idx = _dev_index.get(device)
    if idx is None:
        idx = torch.cuda.current_device() if device is None else torch.device(device).index
        if idx is None:
            idx = torch.cuda.current_device()            # ("cuda" without an index: not cached)
        elif device is not None:
            _dev_index[device] = idx
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(idx))


def ptr_array(tensors, n=None):
    n = n or len(tensors)
    arr = (C.c_void_p * n)()
    for i, t in enumerate(tensors):
        arr[i] = 0 if t is None else t.data_ptr()
    return arr
