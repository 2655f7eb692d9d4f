"""ctypes declarations of include/viorb.h and of the headers it includes, viorb_global_ba_se3.h, viorb_two_view.h and viorb_sim3.h (kept 1:1; tests/test_host_hooks.py checks that every
declared entry point of viorb.h is exported, has a signature here and that the argument counts agree; tests/test_global_ba_se3_ref.py
does the same for SIGNATURES_GLOBAL_BA_SE3, tests/test_two_view_ref.py for SIGNATURES_TWO_VIEW, tests/test_sim3_ref.py for SIGNATURES_SIM3,
tests/test_sim3_match_ref.py for SIGNATURES_SIM3_MATCH, tests/test_kf_culling_ref.py for SIGNATURES_CULLING, tests/test_reloc_ref.py for
SIGNATURES_RELOCALIZATION, tests/test_local_map_ref.py for SIGNATURES_LOCAL_MAP, tests/test_covis_ref.py for SIGNATURES_COVISIBILITY, tests/test_map_correction_ref.py for SIGNATURES_MAP_CORRECTION,
tests/test_kf_removal_ref.py for SIGNATURES_KF_REMOVAL, tests/test_map_fusion_ref.py for SIGNATURES_MAP_FUSION)."""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("VIORB_LIBRARY") or os.path.join(_HERE, "libviorb_hip.so")      # VIORB_LIBRARY: another build of the library (kernel experiments)

KP_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("size", "f4"), ("angle", "f4"),
                     ("response", "f4"), ("octave", "i4"), ("class_id", "i4")])

VIORB_OK, ERR_INVALID_ARG, ERR_NO_DEVICE, ERR_HIP, ERR_CAPACITY, ERR_UNSUPPORTED = 0, -1, -2, -3, -4, -5
VI_INVALID, VI_DEGENERATE, PREINT_NO_CLAMP = 1, 2, 1          # viorb_vi_init status codes; viorb_preintegrate_intervals flag


class ViorbError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("viorb error %d: %s" % (code, msg))
        self.code = code


class FrontendConfig(C.Structure):
    _fields_ = [("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("cam", C.c_double * 16), ("gravity", C.c_double * 3),
                ("scale_factors", C.c_float * 16), ("inv_level_sigma2", C.c_float * 16),
                ("nlevels", C.c_int32), ("check_orientation", C.c_int32),
                ("gyr_meas_cov", C.c_double), ("acc_meas_cov", C.c_double), ("acc_bias_rw2", C.c_double),
                ("dist_coef", C.c_float * 5), ("reserved0", C.c_int32)]


class LbaWindow(C.Structure):
    """viorb_lba_window (include/viorb.h): the arguments of one viorb_local_ba_navstate call + its status."""
    _fields_ = [("kfs", C.c_void_p), ("nk", C.c_int32), ("n_local", C.c_int32), ("prev_kf", C.c_int32), ("preint", C.c_void_p),
                ("points", C.c_void_p), ("np", C.c_int32), ("edge_idx", C.c_void_p), ("edge_obs", C.c_void_p), ("ne", C.c_int32),
                ("gw", C.c_void_p), ("cam", C.c_void_p), ("stop", C.c_void_p), ("kfs_out", C.c_void_p), ("points_out", C.c_void_p),
                ("erase", C.c_void_p), ("info", C.c_void_p), ("status", C.c_int32)]


class LbaSe3Window(C.Structure):
    """viorb_lba_se3_window (include/viorb.h)."""
    _fields_ = [("kfs", C.c_void_p), ("nk", C.c_int32), ("n_local", C.c_int32), ("points", C.c_void_p), ("np", C.c_int32),
                ("edge_idx", C.c_void_p), ("edge_obs", C.c_void_p), ("ne", C.c_int32), ("intr5", C.c_void_p), ("stop", C.c_void_p),
                ("kfs_out", C.c_void_p), ("points_out", C.c_void_p), ("erase", C.c_void_p), ("info", C.c_void_p), ("status", C.c_int32)]


class ExtractorParams(C.Structure):
    _fields_ = [("nfeatures", C.c_int32), ("scale_factor", C.c_float), ("nlevels", C.c_int32),
                ("ini_th_fast", C.c_int32), ("min_th_fast", C.c_int32)]


class VocabularyFlat(C.Structure):
    """viorb_vocabulary_flat (include/viorb.h)."""
    _fields_ = [("n_nodes", C.c_int32), ("k", C.c_int32), ("L", C.c_int32), ("n_words", C.c_int32), ("child_start", C.c_void_p),
                ("child_ids", C.c_void_p), ("word_id", C.c_void_p), ("desc", C.c_void_p), ("weight", C.c_void_p)]


class MappingCamera(C.Structure):
    """viorb_mapping_camera (include/viorb.h)."""
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("mb", C.c_float), ("mbf", C.c_float),
                ("scale_factor", C.c_float), ("nlevels", C.c_int32), ("scale_factors", C.c_float * 16), ("level_sigma2", C.c_float * 16)]


class ViInitConfig(C.Structure):
    """viorb_vi_init_config (include/viorb.h)."""
    _fields_ = [("Tbc", C.c_double * 16), ("g", C.c_double), ("gyr_meas_cov", C.c_double), ("acc_meas_cov", C.c_double)]


class GbaConfig(C.Structure):
    """viorb_gba_config (include/viorb.h)."""
    _fields_ = [("iterations", C.c_int32), ("robust", C.c_int32)]


class EgConfig(C.Structure):
    """viorb_eg_config (include/viorb_essential_graph.h)."""
    _fields_ = [("iterations", C.c_int32), ("fix_scale", C.c_int32)]


class TwoViewConfig(C.Structure):
    """viorb_two_view_config (include/viorb_two_view.h)."""
    _fields_ = [("sigma", C.c_float), ("iterations", C.c_int32), ("min_parallax_deg", C.c_float), ("min_triangulated", C.c_int32),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float)]


TWO_VIEW_OUTPUT_FIELDS = ("status", "reason", "n_matches", "scores", "best_iter", "H21", "F21", "inliers_h", "inliers_f", "R21", "t21", "P3D",
                          "triangulated", "n_hyp", "hyp_n_good", "hyp_parallax", "hyp_R", "hyp_t")


class TwoViewOutputs(C.Structure):
    """viorb_two_view_outputs (include/viorb_two_view.h)."""
    _fields_ = [(n, C.c_void_p) for n in TWO_VIEW_OUTPUT_FIELDS]


class Sim3Inputs(C.Structure):
    """viorb_sim3_inputs (include/viorb_sim3.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("X1c", "X2c", "sigma2_1", "sigma2_2", "K1", "K2", "n")] + [("cap", C.c_int32)]


class Sim3OptInputs(C.Structure):
    """viorb_sim3_opt_inputs (include/viorb_sim3.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("S12", "X1c", "X2c", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2", "valid", "K1", "K2", "n")] + [("cap", C.c_int32)]


class Sim3Config(C.Structure):
    """viorb_sim3_config (include/viorb_sim3.h)."""
    _fields_ = [("iterations", C.c_int32), ("min_inliers", C.c_int32), ("fix_scale", C.c_int32), ("iterations_per_call", C.c_int32)]


SIM3_OUTPUT_FIELDS = ("status", "iterations_done", "best_inliers", "best_iter", "R12", "t12", "s12", "T12", "n_inliers", "inliers")


class Sim3Outputs(C.Structure):
    """viorb_sim3_outputs (include/viorb_sim3.h)."""
    _fields_ = [(n, C.c_void_p) for n in SIM3_OUTPUT_FIELDS]


class S3mKeyframes(C.Structure):
    """viorb_s3m_keyframes (include/viorb_sim3_match.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("kps", "desc", "count", "cell_start", "cell_idx")] + [("cap", C.c_int32)]


class S3mSide(C.Structure):
    """viorb_s3m_side (include/viorb_sim3_match.h)."""
    _fields_ = [("kf", S3mKeyframes)] + [(n, C.c_void_p) for n in ("pose12", "has_point", "pts_f", "pts_desc", "already")]


class RelocConfig(C.Structure):
    """viorb_reloc_config (include/viorb_relocalization.h)."""
    _fields_ = [("min_good", C.c_int32), ("accept", C.c_int32), ("narrow_above", C.c_int32), ("th_coarse", C.c_float), ("orb_dist_coarse", C.c_int32),
                ("th_narrow", C.c_float), ("orb_dist_narrow", C.c_int32), ("check_orientation", C.c_int32)]


class RelocInputs(C.Structure):
    """viorb_reloc_inputs (include/viorb_relocalization.h)."""
    _fields_ = [("frames", C.POINTER(S3mKeyframes)), ("n_frames", C.c_int32), ("hyp_frame", C.c_void_p), ("uright", C.c_void_p)] \
        + [(n, C.c_void_p) for n in ("pose12", "kf_angle", "kf_valid", "pts_f", "pts_desc", "kf_count")] + [("kcap", C.c_int32)] \
        + [(n, C.c_void_p) for n in ("bow_match", "inlier")]


RELOC_OUTPUT_FIELDS = ("accepted", "n_good", "stage", "counts", "out_pose12", "chi2", "frame_match", "outlier")


class RelocOutputs(C.Structure):
    """viorb_reloc_outputs (include/viorb_relocalization.h)."""
    _fields_ = [(n, C.c_void_p) for n in RELOC_OUTPUT_FIELDS]


SEARCH_INIT_OUTPUT_FIELDS = ("matches21", "matched_distance", "rot_hist", "reason", "xy1", "xy2", "sweeps")


class SearchInitOutputs(C.Structure):
    """viorb_search_init_outputs (include/viorb_search_init.h)."""
    _fields_ = [(n, C.c_void_p) for n in SEARCH_INIT_OUTPUT_FIELDS]


CULL_MAP_INTS = ("batch", "n_kf", "n_cand", "n_kp", "n_pt", "n_obs")
CULL_MAP_ARRAYS = ("kf_start", "kf_flags", "kf_time", "kf_prev", "kf_next", "cur_kf", "vins_inited", "th_depth", "cand_start", "cand_kf", "kp_start",
                   "kp_point", "kp_octave", "kp_depth", "pt_start", "pt_nobs", "pt_bad", "obs_start", "obs")
CULL_RESULT_FIELDS = ("cand_reason", "cand_redundant", "cand_mps", "cand_recounted", "culled_order", "n_culled", "status", "kf_bad", "kf_to_be_erased",
                      "kf_prev_out", "kf_next_out", "kf_repreint", "pt_nobs_out", "pt_bad_out", "obs_alive")


class CullMap(C.Structure):
    """viorb_cull_map (include/viorb_culling.h)."""
    _fields_ = [(n, C.c_int32) for n in CULL_MAP_INTS] + [(n, C.c_void_p) for n in CULL_MAP_ARRAYS]


class CullResult(C.Structure):
    """viorb_cull_result (include/viorb_culling.h)."""
    _fields_ = [(n, C.c_void_p) for n in CULL_RESULT_FIELDS]


LOCAL_MAP_INTS = ("batch", "n_kf", "n_child", "n_kp", "n_pt", "n_obs")
LOCAL_MAP_ARRAYS = ("kf_start", "kf_bad", "kf_parent", "kf_prev", "kf_next", "covis10", "child_start", "child_kf", "kf_by_key", "kp_start", "kp_point",
                    "pt_start", "pt_bad", "obs_start", "obs", "frame_point", "frame_count", "prev_lkf", "prev_n_lkf", "prev_ref_kf")
LOCAL_MAP_RESULT_FIELDS = ("lkf", "n_lkf", "n_voted", "ref_kf", "lpt", "n_lpt", "status", "frame_point_out", "kf_votes")


class LocalMapSnapshot(C.Structure):
    """viorb_local_map_snapshot (include/viorb_local_map.h)."""
    _fields_ = [(n, C.c_int32) for n in LOCAL_MAP_INTS] + [(n, C.c_void_p) for n in LOCAL_MAP_ARRAYS]


class LocalMapResult(C.Structure):
    """viorb_local_map_result (include/viorb_local_map.h)."""
    _fields_ = [(n, C.c_void_p) for n in LOCAL_MAP_RESULT_FIELDS]


COVIS_INTS = ("batch", "n_kf", "n_kp", "n_pt", "n_obs", "n_conn", "n_ord", "n_target")
COVIS_ARRAYS = ("kf_start", "kf_by_key", "kf_flags", "kf_parent", "kp_start", "kp_point", "pt_start", "pt_bad", "obs_start", "obs",
                "conn_start", "conn_kf", "conn_w", "ord_start", "ord_kf", "ord_w", "target_start", "target_kf")
COVIS_RESULT_REQUIRED = ("conn_kf_out", "conn_w_out", "conn_n_out", "ord_kf_out", "ord_w_out", "ord_n_out", "status")
COVIS_RESULT_FIELDS = COVIS_RESULT_REQUIRED + ("need", "kf_parent_out", "kf_flags_out", "kf_touched", "t_observers", "t_max_kf", "t_max_w", "t_added",
                                               "t_parent", "loop_conn", "n_loop_conn")


class CovisMap(C.Structure):
    """viorb_covis_map (include/viorb_covisibility.h)."""
    _fields_ = [(n, C.c_int32) for n in COVIS_INTS] + [(n, C.c_void_p) for n in COVIS_ARRAYS]


class CovisResult(C.Structure):
    """viorb_covis_result (include/viorb_covisibility.h)."""
    _fields_ = [(n, C.c_void_p) for n in COVIS_RESULT_FIELDS]


KFR_INTS = ("batch", "n_kf", "n_kp", "n_pt", "n_obs", "n_conn", "n_ord", "n_op")
KFR_ARRAYS = ("kf_start", "kf_by_key", "kf_flags", "kf_parent", "kf_prev", "kf_next", "kf_pose12", "kp_start", "kp_point",
              "pt_start", "pt_bad", "pt_nobs", "pt_ref", "obs_start", "obs", "conn_start", "conn_kf", "conn_w", "ord_start", "ord_kf", "ord_w",
              "op_start", "op_kf", "op_kind")
KFR_RESULT_REQUIRED = COVIS_RESULT_REQUIRED
KFR_RESULT_FIELDS = KFR_RESULT_REQUIRED + ("kf_parent_out", "kf_flags_out", "kf_prev_out", "kf_next_out", "kf_repreint", "kf_Tcp_out", "kf_touched",
                                           "pt_nobs_out", "pt_bad_out", "obs_alive", "pt_ref_out", "kp_point_out",
                                           "op_reason", "op_children", "op_fallback", "op_rebuilt", "op_points_bad")


class KfrMap(C.Structure):
    """viorb_kfr_map (include/viorb_kf_removal.h)."""
    _fields_ = [(n, C.c_int32) for n in KFR_INTS] + [(n, C.c_void_p) for n in KFR_ARRAYS]


class KfrResult(C.Structure):
    """viorb_kfr_result (include/viorb_kf_removal.h)."""
    _fields_ = [(n, C.c_void_p) for n in KFR_RESULT_FIELDS]


FUSE_INTS = ("batch", "n_kf", "n_kp", "n_pt", "n_obs", "n_call", "n_list", "n_feat", "n_op", "n_obs_out")
FUSE_ARRAYS = ("kf_start", "kf_by_key", "kf_bad", "kp_start", "kp_point", "kp_octave", "kp_stereo", "pt_start", "pt_bad", "pt_nobs", "pt_found", "pt_visible",
               "obs_start", "obs", "obs_feat", "call_start", "call_kf", "call_kind", "call_list", "call_n", "call_feat", "call_op",
               "list_point", "op_feat", "obs_out_start")
FUSE_RESULT_REQUIRED = ("status", "kp_point_out", "pt_bad_out", "pt_nobs_out", "obs_start_out", "obs_out", "obs_feat_out")
FUSE_RESULT_FIELDS = FUSE_RESULT_REQUIRED + ("need", "pt_found_out", "pt_visible_out", "pt_replaced_out", "pt_dirty", "obs_touched",
                                             "dirty_obs_start", "dirty_obs_kf", "dirty_obs_feat", "op_reason", "op_other", "call_nfused")


class FuseMap(C.Structure):
    """viorb_fuse_map (include/viorb_map_fusion.h)."""
    _fields_ = [(n, C.c_int32) for n in FUSE_INTS] + [(n, C.c_void_p) for n in FUSE_ARRAYS]


class FuseResult(C.Structure):
    """viorb_fuse_result (include/viorb_map_fusion.h)."""
    _fields_ = [(n, C.c_void_p) for n in FUSE_RESULT_FIELDS]


CORRECT_LOOP_INTS = ("batch", "n_kf", "n_kp", "n_pt", "n_obs", "n_conn")
CORRECT_LOOP_ARRAYS = ("kf_start", "kf_by_key", "kp_start", "kp_point", "pt_start", "pt_bad", "obs_start", "obs", "pose12", "pts_f", "pt_ref",
                       "pt_corrected_by", "cur_kf", "cur_id", "Scw8", "conn_start", "conn_kf")
CORRECT_LOOP_RESULT_FIELDS = ("status", "n_member", "member_kf", "Scw_f12", "Scw_out", "Smeas_out", "pose12_out", "Ow_out", "pts_f_out",
                              "pt_corrected_by_out", "pt_corrected_ref_out", "pt_touched")


APPLY_GBA_INTS = ("batch", "n_kf", "n_child", "n_origin", "n_pt")
APPLY_GBA_ARRAYS = ("kf_start", "child_start", "child_kf", "origin_start", "origin_kf", "kf_in_gba", "pose12", "TcwGBA12", "ns22", "nsGBA22",
                    "pt_start", "pt_bad", "pt_in_gba", "Pw", "PosGBA", "pt_ref")
APPLY_GBA_RESULT_FIELDS = ("status", "pose12_out", "ns22_out", "TcwBef_out", "nsBef_out", "TcwGBA_out", "nsGBA_out", "kf_in_gba_out", "kf_reached", "Pw_out", "pt_code")


class ApplyGbaMap(C.Structure):
    """viorb_apply_gba_map (include/viorb_map_correction.h)."""
    _fields_ = [(n, C.c_int32) for n in APPLY_GBA_INTS] + [(n, C.c_void_p) for n in APPLY_GBA_ARRAYS]


class ApplyGbaResult(C.Structure):
    """viorb_apply_gba_result (include/viorb_map_correction.h)."""
    _fields_ = [(n, C.c_void_p) for n in APPLY_GBA_RESULT_FIELDS]


class CorrectLoopMap(C.Structure):
    """viorb_correct_loop_map (include/viorb_map_correction.h)."""
    _fields_ = [(n, C.c_int32) for n in CORRECT_LOOP_INTS] + [(n, C.c_void_p) for n in CORRECT_LOOP_ARRAYS]


class CorrectLoopResult(C.Structure):
    """viorb_correct_loop_result (include/viorb_map_correction.h)."""
    _fields_ = [(n, C.c_void_p) for n in CORRECT_LOOP_RESULT_FIELDS]


class TrackerConfig(C.Structure):
    """viorb_tracker_config (include/viorb.h)."""
    _fields_ = [("extractor", ExtractorParams), ("frontend", FrontendConfig), ("width", C.c_int32), ("height", C.c_int32), ("batch", C.c_int32),
                ("device", C.c_int32), ("th_projection", C.c_float), ("track_local_map", C.c_int32), ("local_frames", C.c_int32),
                ("compute_marg", C.c_int32), ("max_steps_ahead", C.c_int32), ("synth_plane_z0", C.c_double)]


class TrackerInputs(C.Structure):
    """viorb_tracker_inputs (include/viorb.h)."""
    _fields_ = [("d_images", C.c_void_p), ("image_stride", C.c_int32), ("image_pitch_bytes", C.c_size_t), ("d_imu", C.c_void_p), ("n_imu", C.c_int32),
                ("d_t_cur", C.c_void_p), ("d_map_updated", C.c_void_p), ("d_recent_reloc", C.c_void_p), ("d_t_next_last", C.c_void_p),
                ("d_reset_ns", C.c_void_p), ("d_reset_marg", C.c_void_p), ("d_synth_pose12", C.c_void_p), ("h_images", C.c_void_p)]


class TrackerResults(C.Structure):
    """viorb_tracker_results (include/viorb.h)."""
    _fields_ = [("cap", C.c_int32)] + [(n, C.c_void_p) for n in (
        "state", "status", "nmatches", "n_map", "n_loc", "inliers", "n_obs", "n_obs2", "cur_match", "loc_match", "last_count",
        "info", "info2", "pred_ns", "ns_stage1", "ns_stage2", "final_ns", "final_marg", "last_ns",
        "outlier_cur", "outlier_cur2", "last_flags", "last_Pw", "last_pts_f", "extractor")]


vp, i32, f32, sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
PP = C.POINTER
# name -> (restype, argtypes); mirrors include/viorb.h
SIGNATURES = {
    "viorb_abi_version": (i32, []),
    "viorb_last_error": (C.c_char_p, []),
    "viorb_device_count": (i32, []),
    "viorb_extractor_create": (i32, [PP(ExtractorParams), i32, i32, PP(vp)]),
    "viorb_extractor_destroy": (i32, [vp]),
    "viorb_extractor_tables": (i32, [vp, vp, vp, vp, vp, vp]),
    "viorb_extractor_max_keypoints": (i32, [vp, PP(i32)]),
    "viorb_extractor_max_keypoints_for": (i32, [vp, i32, i32, PP(i32)]),
    "viorb_extractor_fast_launch_images": (i32, [i32]),
    "viorb_extract": (i32, [vp, vp, i32, i32, i32, vp, vp, i32, PP(i32)]),
    "viorb_extract_batch_device": (i32, [vp, vp, i32, i32, i32, i32, sz, vp]),
    "viorb_extractor_results_device": (i32, [vp, PP(vp), PP(vp), PP(vp), PP(vp), PP(i32)]),
    "viorb_extractor_download": (i32, [vp, i32, vp, vp, i32, PP(i32)]),
    "viorb_extractor_level_device": (i32, [vp, i32, i32, i32, PP(vp), PP(i32), PP(i32), PP(i32)]),
    "viorb_extractor_level_download": (i32, [vp, i32, i32, i32, vp, PP(i32), PP(i32)]),
    "viorb_stereo_match_device": (i32, [vp, i32, vp, i32, i32, f32, f32, vp, vp, vp, vp]),
    "viorb_stereo_match": (i32, [vp, vp, f32, f32, vp, vp, i32, PP(i32)]),
    "viorb_extractor_debug_level_points": (i32, [vp, i32, i32, i32, vp, i32, PP(i32)]),
    "viorb_frontend_create": (i32, [PP(FrontendConfig), i32, i32, i32, PP(vp)]),
    "viorb_frontend_search_capacity": (i32, []),
    "viorb_frontend_destroy": (i32, [vp]),
    "viorb_frontend_capacity": (i32, [vp, vp, vp]),
    "viorb_frontend_grid_device": (i32, [vp, vp, vp, i32, vp, vp, vp]),
    "viorb_frontend_undistort_device": (i32, [vp, vp, vp, i32, vp, vp]),
    "viorb_undistort_points": (i32, [vp, i32, vp, vp, vp]),
    "viorb_image_bounds": (i32, [i32, i32, vp, vp, vp]),
    "viorb_frontend_imu_predict_device": (i32, [vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp]),
    "viorb_frontend_search_projection_device": (i32, [vp] * 12 + [f32, i32, vp, vp, vp, vp]),
    "viorb_frontend_search_projection_retry_device": (i32, [vp] * 12 + [f32, i32, i32, vp, vp, vp, vp]),
    "viorb_frontend_set_pose_shape": (i32, [i32, i32]),
    "viorb_frontend_search_local_points_device": (i32, [vp] * 11 + [i32, f32, f32, vp, i32, vp, vp, vp, vp, vp]),
    "viorb_frontend_search_local_points_stereo_device": (i32, [vp] * 5 + [f32] + [vp] * 7 + [i32, f32, f32, vp, i32, vp, vp, vp, vp, vp, vp]),
    "viorb_frontend_build_observations_device": (i32, [vp, vp, vp, vp, vp, i32, vp, vp, vp, vp]),
    "viorb_frontend_pose_opt_device": (i32, [vp, i32, i32] + [vp] * 9 + [i32] + [vp] * 7),
    "viorb_frontend_pose_opt_se3_device": (i32, [vp, vp, vp, vp, C.c_double, i32, vp, vp, vp, vp]),
    "viorb_pose_opt_se3": (i32, [vp, vp, vp, i32, vp, vp, vp]),
    "viorb_local_ba_navstate": (i32, [vp, i32, i32, i32, vp, vp, i32, vp, vp, i32] + [vp] * 7),
    "viorb_local_ba_navstate_batch": (i32, [vp, i32, i32]),
    "viorb_local_ba_set_device": (i32, [i32]),
    "viorb_local_ba_se3_batch": (i32, [vp, i32, i32]),
    "viorb_local_ba_se3": (i32, [vp, i32, i32, vp, i32, vp, vp, i32] + [vp] * 6),
    "viorb_vocabulary_create": (i32, [i32, i32, vp, vp, vp, vp, vp, PP(vp)]),
    "viorb_vocabulary_destroy": (i32, [vp]),
    "viorb_vocabulary_read_file": (i32, [C.c_char_p, i32, PP(VocabularyFlat)]),
    "viorb_vocabulary_flat_free": (None, [PP(VocabularyFlat)]),
    "viorb_vocabulary_load_text": (i32, [C.c_char_p, PP(vp)]),
    "viorb_vocabulary_load_binary": (i32, [C.c_char_p, PP(vp)]),
    "viorb_vocabulary_save_text": (i32, [C.c_char_p, i32, i32, i32, vp, vp, vp, vp]),
    "viorb_vocabulary_save_binary": (i32, [C.c_char_p, i32, i32, i32, vp, vp, vp, vp]),
    "viorb_bow_transform_device": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, vp, vp]),
    "viorb_bow_transform": (i32, [vp, vp, i32, i32, vp, vp, vp]),
    "viorb_search_by_bow_device": (i32, [vp] * 9 + [i32, i32, f32, i32, vp, vp, vp]),
    "viorb_search_by_bow": (i32, [vp, vp, vp, vp, i32, vp, vp, vp, i32, f32, i32, vp, PP(i32)]),
    "viorb_match_bruteforce_device": (i32, [vp, vp, i32, vp, vp, i32, i32, vp, vp, vp, vp]),
    "viorb_match_bruteforce": (i32, [vp, i32, vp, i32, vp, vp, vp]),
    "viorb_frontend_discard_outliers_device": (i32, [vp, vp, vp, vp, vp, vp, i32, vp, vp, vp]),
    "viorb_frontend_pose_from_navstate_device": (i32, [vp, vp, i32, vp, vp]),
    "viorb_frontend_build_observations2_device": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp]),
    "viorb_synth_local_points_device": (i32, [vp, vp, vp, vp, vp, i32, vp, vp]),
    "viorb_search_for_triangulation_device": (i32, [vp] * 18 + [i32, i32, i32, i32, i32, vp, vp, vp]),
    "viorb_search_for_triangulation": (i32, [vp] * 5 + [i32] + [vp] * 5 + [i32] + [vp] * 6 + [i32, i32, i32, vp, PP(i32)]),
    "viorb_frontend_fuse_device": (i32, [vp] * 12 + [i32, f32, f32, i32, vp, vp, vp]),
    "viorb_fuse": (i32, [vp, vp, vp, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, i32, f32, vp, PP(i32)]),
    "viorb_synth_plane_points_device": (i32, [vp, vp, vp, vp, C.c_double, i32, vp, vp, vp, vp]),
    "viorb_frontend_roll_device": (i32, [vp] * 12 + [i32, i32] + [vp] * 7 + [i32, vp]),
    "viorb_memcpy_dtod_async": (i32, [vp, vp, sz, vp]),
    "viorb_memcpy_dtoh": (i32, [vp, vp, sz]),
    "viorb_memcpy_htod": (i32, [vp, vp, sz]),
    "viorb_frontend_pose_opt_select_device": (i32, [vp, vp, vp, i32] + [vp] * 9 + [i32] + [vp] * 7),
    "viorb_frontend_self_index_device": (i32, [vp, vp, vp, i32, vp, vp]),
    "viorb_tracker_create": (i32, [PP(TrackerConfig), PP(vp)]),
    "viorb_tracker_destroy": (i32, [vp]),
    "viorb_tracker_capacity": (i32, [vp, PP(i32)]),
    "viorb_tracker_bootstrap": (i32, [vp, vp, i32, sz, vp, vp, vp, vp, vp]),
    "viorb_tracker_set_last_points_device": (i32, [vp, vp, vp, vp, vp]),
    "viorb_tracker_step": (i32, [vp, PP(TrackerInputs), vp]),
    "viorb_tracker_sync": (i32, [vp]),
    "viorb_tracker_results_device": (i32, [vp, PP(TrackerResults)]),
    "viorb_tracker_host_stats": (i32, [vp, PP(C.c_double), PP(C.c_double), PP(C.c_longlong), i32]),
    "viorb_profile_enable": (i32, [i32]),
    "viorb_profile_reset": (i32, []),
    "viorb_profile_select": (i32, [C.c_char_p]),
    "viorb_profile_read": (i32, [C.c_char_p, i32, vp, vp, i32, PP(i32)]),
    "viorb_profile_timeline": (i32, [vp, vp, vp, i32, vp]),
    "viorb_descriptor_distance": (i32, [vp, vp]),
    "viorb_search_by_projection_frame": (i32, [vp, vp, i32, vp, vp, vp, vp, i32, vp, i32, vp, vp, vp, f32, i32, vp, PP(i32)]),
    "viorb_search_by_projection_frame_stereo": (i32, [vp, vp, vp, i32, vp, vp, vp, vp, f32, f32, vp, i32, vp, i32, vp, vp, vp, f32, i32, vp, PP(i32)]),
    "viorb_frontend_search_projection_stereo_device": (i32, [vp] * 14 + [f32, f32, f32, i32, i32, vp, vp, vp, vp]),
    "viorb_search_by_projection_points": (i32, [vp, vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, i32, f32, f32, vp, vp, PP(i32), vp]),
    "viorb_search_by_projection_points_stereo": (i32, [vp, vp, vp, f32, i32, vp, vp, vp, vp, i32, vp, vp, vp, i32, f32, f32, vp, vp, PP(i32), vp, vp]),
    "viorb_preintegrate": (i32, [vp, i32, vp, vp, C.c_double, C.c_double, vp]),
    "viorb_pose_opt_vi": (i32, [i32, i32] + [vp] * 8 + [i32, vp, i32] + [vp] * 6),
    "viorb_debug_pvr_edge": (None, [vp] * 7),
    "viorb_debug_proj_edge": (None, [vp] * 5),
    "viorb_debug_prior_edge": (None, [vp] * 5),
    "viorb_debug_update_ns": (None, [vp] * 6),
    "viorb_debug_preint_step": (None, [vp, vp, vp, C.c_double]),
    "viorb_debug_octree_host": (i32, [vp, i32, i32, i32, i32, vp, i32, PP(i32)]),
    "viorb_debug_fast_atan2": (f32, [f32, f32]),
    "viorb_debug_sincos": (None, [f32, PP(f32), PP(f32)]),
    "viorb_triangulate_pairs_device": (i32, [vp] * 15 + [i32, i32] + [vp] * 4),
    "viorb_triangulate_pairs": (i32, [vp] * 5 + [i32] + [vp] * 6 + [i32] + [vp] * 6),
    "viorb_map_points_update_device": (i32, [vp] * 5 + [i32, vp, vp, i32, vp, vp, C.c_int64] + [vp] * 5),
    "viorb_map_points_update": (i32, [vp] * 5 + [i32, vp, vp, i32, vp, vp, C.c_int64] + [vp] * 4),
    "viorb_create_new_map_points_workspace_bytes": (sz, [i32, i32]),
    "viorb_create_new_map_points_device": (i32, [vp, i32] + [vp] * 24 + [i32] * 6 + [vp] * 6 + [sz, vp]),
    "viorb_create_new_map_points": (i32, [vp, i32] + [vp] * 7 + [i32] + [vp] * 15 + [i32] * 3 + [vp] * 3 + [PP(i32)]),
    "viorb_debug_triangulate_pair": (i32, [vp] * 6 + [i32, vp, i32, vp]),
    "viorb_debug_map_point_update": (i32, [vp] * 5 + [i32, vp, vp, i32, vp, vp, C.c_int64] + [vp] * 4),
    "viorb_preintegrate_intervals_device": (i32, [vp, vp, vp, vp, C.c_int64, vp, vp, C.c_double, C.c_double, i32, i32, i32, vp, vp]),
    "viorb_preintegrate_intervals": (i32, [i32, vp, vp, vp, vp, vp, C.c_double, C.c_double, i32, vp]),
    "viorb_optimize_initial_gyro_bias_device": (i32, [PP(ViInitConfig), vp, vp, vp, i32, i32, vp, vp, vp]),
    "viorb_optimize_initial_gyro_bias": (i32, [PP(ViInitConfig), i32, vp, vp, vp, vp]),
    "viorb_vi_init_device": (i32, [PP(ViInitConfig), vp, vp, vp, vp, C.c_int64, vp, vp, i32, i32, vp, vp, vp, vp]),
    "viorb_vi_init": (i32, [PP(ViInitConfig), i32, vp, vp, vp, vp, vp, vp, vp, vp]),
    "viorb_vi_init_apply_device": (i32, [PP(ViInitConfig)] + [vp] * 5 + [C.c_int64] + [vp] * 5 + [i32, i32] + [vp] * 4),
    "viorb_vi_init_apply": (i32, [PP(ViInitConfig), i32, i32] + [vp] * 10),
    "viorb_scale_map_points_device": (i32, [vp] * 5 + [i32, i32, vp]),
    "viorb_debug_vi_init_navstate": (None, [vp, i32, i32, i32] + [vp] * 5),
    "viorb_debug_vi_init_gyro_edge": (None, [vp] * 7),
    "viorb_debug_vi_init_gyro_solve": (i32, [vp, vp]),
    "viorb_debug_vi_init_rows": (None, [vp] * 5 + [C.c_double, vp, vp]),
    "viorb_debug_vi_init_solve": (i32, [vp, vp, i32, i32, vp, vp]),
    "viorb_debug_vi_init_rwi": (i32, [vp, vp]),
    "viorb_global_ba_navstate_workspace_bytes": (sz, [i32, i32, i32]),
    "viorb_global_ba_navstate": (i32, [PP(GbaConfig), vp, i32, vp, vp, vp, vp, i32, vp, vp, i32] + [vp] * 7),
    "viorb_global_ba_navstate_device": (i32, [PP(GbaConfig), vp, i32, vp, vp, vp, vp, i32, vp, vp, i32] + [vp] * 8 + [sz, vp]),
    "viorb_debug_gba_cholesky": (i32, [vp, i32, vp, vp]),
    "viorb_debug_gba_last_trials": (i32, [vp, i32, PP(i32)]),
    "viorb_bow_vector_device": (i32, [vp, vp, vp, i32, i32, vp, vp, vp, vp]),
    "viorb_bow_vector": (i32, [vp, vp, i32, vp, vp, PP(i32)]),
    "viorb_bow_score_device": (i32, [vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, i32, vp, vp]),
    "viorb_bow_score": (i32, [vp, vp, vp, i32, i32, vp, vp, vp, i32, i32, vp, vp, i32, vp]),
    "viorb_kfdb_create": (i32, [i32, i32, i32, PP(vp)]),
    "viorb_kfdb_destroy": (i32, [vp]),
    "viorb_kfdb_add_device": (i32, [vp, vp, vp, vp, i32, i32, PP(i32), vp]),
    "viorb_kfdb_add": (i32, [vp, vp, vp, i32, PP(i32)]),
    "viorb_kfdb_erase": (i32, [vp, i32]),
    "viorb_kfdb_clear": (i32, [vp]),
    "viorb_kfdb_size": (i32, [vp, PP(i32), PP(i32)]),
    "viorb_kfdb_query_workspace_bytes": (sz, [vp, i32]),
    "viorb_kfdb_query_device": (i32, [vp, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, sz, vp]),
    "viorb_kfdb_query": (i32, [vp, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp]),
    "viorb_debug_place_score": (C.c_double, [vp, vp, i32, vp, vp, i32]),
    "viorb_debug_place_select": (i32, [i32, i32, vp, vp, vp, f32, vp, i32, vp, vp, vp]),
}
# mirrors include/viorb_global_ba_se3.h (the header viorb.h includes for the vision-only global bundle adjustment);
# tests/test_global_ba_se3_ref.py checks names and argument counts against it
SIGNATURES_GLOBAL_BA_SE3 = {
    "viorb_global_ba_se3_workspace_bytes": (sz, [i32, i32, i32]),
    "viorb_global_ba_se3": (i32, [PP(GbaConfig), vp, i32, vp, vp, i32, vp, vp, i32] + [vp] * 6),
    "viorb_global_ba_se3_device": (i32, [PP(GbaConfig), vp, i32, vp, vp, i32, vp, vp, i32] + [vp] * 7 + [sz, vp]),
    "viorb_debug_gba_se3_edge": (i32, [vp] * 7),
}

# mirrors include/viorb_two_view.h (the two-view initialiser); tests/test_two_view_ref.py checks names and argument counts against it
_tv_in = [PP(TwoViewConfig), vp, vp, vp, vp, i32, vp]          # cfg, xy1, n1, xy2, n2, cap, matches12
SIGNATURES_TWO_VIEW = {
    "viorb_two_view_draw_sets": (i32, [i32, i32, C.c_uint64, vp]),
    "viorb_two_view_workspace_bytes": (sz, [i32, i32, i32]),
    "viorb_two_view_init_device": (i32, _tv_in + [vp, i32, PP(TwoViewOutputs), vp, sz, vp]),
    "viorb_two_view_init": (i32, [PP(TwoViewConfig), vp, i32, vp, i32, vp, vp, PP(TwoViewOutputs)]),
    "viorb_two_view_hypotheses_device": (i32, _tv_in + [vp, i32, vp, vp, vp, vp, vp, sz, vp]),
    "viorb_two_view_score_device": (i32, _tv_in + [i32, vp, vp, vp, vp, vp, vp, sz, vp]),
    "viorb_two_view_reconstruct_device": (i32, _tv_in + [i32, vp, vp, vp, PP(TwoViewOutputs), vp, sz, vp]),
    "viorb_debug_two_view_hypothesis": (i32, [i32, vp, vp, vp, vp]),
    "viorb_debug_two_view_denormalise": (i32, [i32, vp, vp, vp, vp, vp]),
    "viorb_debug_two_view_normalise": (i32, [vp, i32, vp]),
    "viorb_debug_two_view_chi2": (i32, [i32, vp, vp, vp, f32, vp, vp]),
    "viorb_debug_two_view_decompose": (i32, [i32, vp, vp, vp, vp, vp]),
    "viorb_debug_two_view_check_rt": (i32, [vp, vp, vp, vp, f32, vp, vp]),
    "viorb_debug_two_view_parallax": (f32, [vp, i32]),
    "viorb_debug_two_view_accept": (i32, [i32, vp, vp, i32, f32, i32, vp]),
}

# mirrors include/viorb_sim3.h (the Sim3 RANSAC solver); tests/test_sim3_ref.py checks names and argument counts against it
_s3_in = [PP(Sim3Inputs), PP(Sim3Config)]
SIGNATURES_SIM3 = {
    "viorb_sim3_draw_sets": (i32, [i32, i32, C.c_uint64, vp]),
    "viorb_sim3_ransac_iterations": (i32, [i32, C.c_double, i32, i32]),
    "viorb_sim3_workspace_bytes": (sz, [i32, i32, i32]),
    "viorb_sim3_hypotheses_device": (i32, _s3_in + [vp, i32, vp, vp, vp, vp, vp, sz, vp]),
    "viorb_sim3_inliers_device": (i32, _s3_in + [i32, vp, vp, vp, vp, vp, vp, sz, vp]),
    "viorb_sim3_select_device": (i32, [PP(Sim3Config), vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp]),
    "viorb_sim3_ransac_device": (i32, _s3_in + [vp, vp, vp, vp, i32, PP(Sim3Outputs), vp, sz, vp]),
    "viorb_sim3_ransac": (i32, [PP(Sim3Config), vp, vp, vp, vp, vp, vp, i32, vp, i32, i32, i32, PP(Sim3Outputs)]),
    "viorb_optimize_sim3_device": (i32, [PP(Sim3OptInputs), f32, i32, i32, vp, vp, vp, vp, vp]),
    "viorb_optimize_sim3": (i32, [vp, f32, i32] + [vp] * 9 + [i32, vp, vp, vp, vp]),
    "viorb_debug_sim3_exp": (i32, [vp, vp, vp, vp]),
    "viorb_debug_sim3_edges": (i32, [vp] * 7 + [i32, vp, vp]),
    "viorb_debug_sim3_horn": (i32, [vp, vp, i32, vp, vp, vp]),
    "viorb_debug_sim3_inlier": (i32, [vp, vp, f32, vp, vp, vp, vp, f32, f32, vp, vp]),
    "viorb_debug_sim3_select": (i32, [vp, i32, i32, i32, i32, i32, i32, i32, vp]),
}

# mirrors include/viorb_sim3_match.h (the Sim3 matchers); tests/test_sim3_match_ref.py checks names and argument counts against it
_cam = [PP(MappingCamera), vp, f32]                             # cam, bounds4, th
SIGNATURES_SIM3_MATCH = {
    "viorb_sim3_match_workspace_bytes": (sz, [i32, i32, i32]),
    "viorb_sim3_match_shape": (i32, [vp]),
    "viorb_keyframe_grid_device": (i32, [vp, vp, i32, i32, vp, vp, vp, vp]),
    "viorb_keyframe_grid": (i32, [vp, i32, vp, vp, vp]),
    "viorb_search_by_sim3_device": (i32, [PP(S3mSide), PP(S3mSide), vp, vp, vp] + _cam + [i32] + [vp] * 7 + [sz, vp]),
    "viorb_search_by_sim3": (i32, [vp, vp, i32, vp, vp, vp, vp, vp] * 2 + [vp, vp, f32] + _cam + [vp] * 6),
    "viorb_search_by_projection_sim3_device": (i32, [PP(S3mKeyframes), vp, vp, vp, vp, vp, i32, vp] + _cam + [i32, vp, vp, vp, vp, sz, vp]),
    "viorb_search_by_projection_sim3": (i32, [vp, vp, i32, vp, vp, vp, vp, i32, vp] + _cam + [vp, vp, vp]),
    "viorb_fuse_sim3_device": (i32, [PP(S3mKeyframes), vp, vp, vp, vp, i32, i32] + _cam + [i32, vp, vp, vp, vp, sz, vp]),
    "viorb_fuse_sim3": (i32, [vp, vp, i32, vp, vp, vp, vp, i32] + _cam + [vp, vp, vp]),
    "viorb_debug_sim3_decompose": (i32, [vp, vp]),
    "viorb_debug_sim3_pair": (i32, [vp, vp, f32, vp]),
    "viorb_debug_sim3_project": (i32, [i32, vp, vp, vp, vp] + _cam + [vp, vp]),
    "viorb_debug_claim_in_order": (i32, [vp, vp, i32, i32, vp, i32, vp, vp]),
}

# mirrors include/viorb_search_init.h (the monocular matcher and the scene depth); tests/test_search_init_ref.py checks names and argument
# counts against it
SIGNATURES_SEARCH_INIT = {
    "viorb_search_init_workspace_bytes": (sz, [i32, i32]),
    "viorb_search_init_shape": (i32, [vp]),
    "viorb_search_for_initialization_device": (i32, [vp, vp, vp, PP(S3mKeyframes), vp, i32, i32, vp, i32, f32, i32, vp, vp, PP(SearchInitOutputs),
                                                     vp, sz, vp]),
    "viorb_search_for_initialization": (i32, [vp, vp, i32, vp, vp, i32, vp, vp, i32, f32, i32, vp, vp, PP(SearchInitOutputs)]),
    "viorb_scene_median_depth_device": (i32, [vp, vp, vp, vp, i32, i32, i32, vp, vp, vp]),
    "viorb_scene_median_depth": (i32, [vp, vp, vp, i32, i32, vp, vp]),
    "viorb_debug_search_init_ordered": (i32, [vp, vp, i32, i32, i32, f32, vp, vp, vp, vp, vp, vp]),
    "viorb_debug_search_init_window": (i32, [vp, i32, vp, vp, vp, f32, f32, f32, i32, vp, vp]),
    "viorb_debug_scene_depth": (f32, [vp, vp]),
}

# mirrors include/viorb_essential_graph.h (the essential-graph optimisation); tests/test_essential_graph_ref.py checks names and argument
# counts against it
SIGNATURES_ESSENTIAL_GRAPH = {
    "viorb_essential_graph_workspace_bytes": (sz, [i32, i32, i32]),
    "viorb_optimize_essential_graph": (i32, [PP(EgConfig), vp, vp, vp, i32, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp]),
    "viorb_optimize_essential_graph_device": (i32, [PP(EgConfig), vp, vp, vp, i32, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, sz, vp]),
    "viorb_debug_sim3_log": (i32, [vp, vp]),
    "viorb_debug_essential_graph_edge": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, vp]),
}

# mirrors include/viorb_culling.h (key-frame and map-point culling); tests/test_kf_culling_ref.py checks names and argument counts against it
SIGNATURES_CULLING = {
    "viorb_key_frame_culling_workspace_bytes": (sz, [i32, i32, i32, i32, i32]),
    "viorb_key_frame_culling_device": (i32, [PP(CullMap), i32, PP(CullResult), vp, sz, vp]),
    "viorb_key_frame_culling": (i32, [PP(CullMap), i32, PP(CullResult)]),
    "viorb_key_frame_culling_shape": (i32, [vp]),
    "viorb_map_point_culling_device": (i32, [vp] * 7 + [i32, i32, i32, vp, vp]),
    "viorb_map_point_culling": (i32, [vp] * 5 + [i32, i32, i32, vp]),
    "viorb_debug_key_frame_culling_host": (i32, [PP(CullMap), i32, PP(CullResult)]),
    "viorb_debug_map_point_code": (i32, [i32] * 7),
}

# mirrors include/viorb_relocalization.h (the relocalisation matcher and the refine cascade); tests/test_reloc_ref.py checks names and
# argument counts against it
SIGNATURES_RELOCALIZATION = {
    "viorb_relocalization_workspace_bytes": (sz, [i32, i32, i32]),
    "viorb_search_by_projection_reloc_device": (i32, [PP(S3mKeyframes), i32] + [vp] * 8 + [i32, vp] + _cam + [i32, i32, i32, vp, vp, vp, vp, sz, vp]),
    "viorb_search_by_projection_reloc": (i32, [vp, vp, i32] + [vp] * 6 + [i32, vp] + _cam + [i32, i32, vp, vp, vp]),
    "viorb_reloc_config_default": (i32, [PP(RelocConfig)]),
    "viorb_relocalization_refine_workspace_bytes": (sz, [i32, i32, i32, i32]),
    "viorb_relocalization_refine_device": (i32, [vp, PP(RelocInputs), PP(RelocConfig), PP(MappingCamera), vp, C.c_double, i32, PP(RelocOutputs), vp, sz, vp]),
    "viorb_relocalization_refine": (i32, [vp, vp, vp, i32, vp, vp, vp, vp, vp, i32, vp, vp, PP(RelocConfig), PP(MappingCamera), vp, C.c_double] + [vp] * 8),
    "viorb_relocalization_shape": (i32, [vp]),
    "viorb_debug_reloc_project": (i32, [vp, vp] + _cam + [vp, vp]),
    "viorb_debug_reloc_match": (i32, [vp, vp, i32, i32, vp, i32, i32, i32, vp, vp, vp, vp, vp]),
    "viorb_debug_reloc_decide": (i32, [PP(RelocConfig), i32, i32, i32]),
}

# mirrors include/viorb_local_map.h (Tracking::UpdateLocalMap and the packing of its points); tests/test_local_map_ref.py checks names and
# argument counts against it
SIGNATURES_LOCAL_MAP = {
    "viorb_update_local_map_workspace_bytes": (sz, [i32, i32, i32]),
    "viorb_update_local_map_device": (i32, [PP(LocalMapSnapshot), PP(LocalMapResult), i32, i32, i32, vp, sz, vp]),
    "viorb_update_local_map": (i32, [PP(LocalMapSnapshot), PP(LocalMapResult), i32, i32, i32]),
    "viorb_update_local_map_shape": (i32, [vp]),
    "viorb_local_points_gather_workspace_bytes": (sz, [i32]),
    "viorb_local_points_gather_device": (i32, [PP(LocalMapSnapshot), PP(LocalMapResult), i32, i32] + [vp] * 8 + [sz, vp]),
    "viorb_debug_update_local_map_host": (i32, [PP(LocalMapSnapshot), PP(LocalMapResult), i32, i32, i32]),
}

# mirrors include/viorb_covisibility.h (KeyFrame::UpdateConnections for ordered targets); tests/test_covis_ref.py checks names and
# argument counts against it
SIGNATURES_COVISIBILITY = {
    "viorb_update_connections_workspace_bytes": (sz, [i32, i32, i32, i32]),
    "viorb_update_connections_device": (i32, [PP(CovisMap), PP(CovisResult), i32, i32, vp, sz, vp]),
    "viorb_update_connections": (i32, [PP(CovisMap), PP(CovisResult), i32, i32]),
    "viorb_update_connections_shape": (i32, [vp]),
    "viorb_debug_update_connections_host": (i32, [PP(CovisMap), PP(CovisResult), i32, i32]),
}

# mirrors include/viorb_map_correction.h (the propagation of LoopClosing::CorrectLoop); tests/test_map_correction_ref.py checks names and
# argument counts against it
SIGNATURES_MAP_CORRECTION = {
    "viorb_correct_loop_workspace_bytes": (sz, [i32, i32, i32, i32]),
    "viorb_correct_loop_device": (i32, [PP(CorrectLoopMap), PP(MappingCamera), PP(CorrectLoopResult), vp, sz, vp]),
    "viorb_correct_loop": (i32, [PP(CorrectLoopMap), PP(MappingCamera), PP(CorrectLoopResult)]),
    "viorb_correct_loop_shape": (i32, [vp]),
    "viorb_debug_correct_loop_host": (i32, [PP(CorrectLoopMap), PP(MappingCamera), PP(CorrectLoopResult)]),
    "viorb_apply_global_ba_workspace_bytes": (sz, [i32, i32]),
    "viorb_apply_global_ba_device": (i32, [PP(ApplyGbaMap), vp, PP(ApplyGbaResult), vp, sz, vp]),
    "viorb_apply_global_ba": (i32, [PP(ApplyGbaMap), vp, PP(ApplyGbaResult)]),
    "viorb_apply_global_ba_shape": (i32, [vp]),
    "viorb_debug_apply_global_ba_host": (i32, [PP(ApplyGbaMap), vp, PP(ApplyGbaResult)]),
}

# mirrors include/viorb_kf_removal.h (KeyFrame::SetBadFlag / SetErase for ordered operations); tests/test_kf_removal_ref.py checks names
# and argument counts against it
SIGNATURES_KF_REMOVAL = {
    "viorb_remove_key_frames_workspace_bytes": (sz, [i32, i32, i32, i32]),
    "viorb_remove_key_frames_device": (i32, [PP(KfrMap), PP(KfrResult), i32, vp, sz, vp]),
    "viorb_remove_key_frames": (i32, [PP(KfrMap), PP(KfrResult), i32]),
    "viorb_remove_key_frames_shape": (i32, [vp]),
    "viorb_debug_remove_key_frames_host": (i32, [PP(KfrMap), PP(KfrResult), i32]),
}

# mirrors include/viorb_map_fusion.h (the fuse searches' results applied to the map); tests/test_map_fusion_ref.py checks names and
# argument counts against it
SIGNATURES_MAP_FUSION = {
    "viorb_apply_fuse_workspace_bytes": (sz, [i32, i32, i32, i32, i32]),
    "viorb_apply_fuse_device": (i32, [PP(FuseMap), PP(FuseResult), vp, sz, vp]),
    "viorb_apply_fuse": (i32, [PP(FuseMap), PP(FuseResult)]),
    "viorb_apply_fuse_shape": (i32, [vp]),
    "viorb_fuse_merge_descriptors_device": (i32, [vp, vp, vp, vp, i32, vp]),
    "viorb_debug_apply_fuse_host": (i32, [PP(FuseMap), PP(FuseResult)]),
}

_lib = None


def lib():
    """Load libviorb_hip.so. Raises (never falls back) when it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise ImportError("%s not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc, gfx950). viorb_amd has no CPU fallback." % SO_PATH)
        # One HIP runtime per process: PyTorch ships its own libamdhip64 (same SONAME as /opt/rocm's).
        # If torch is going to be used in this process it must be loaded FIRST so that libviorb_hip.so
        # binds to the runtime already in memory; loading ours first makes torch open a second runtime
        # that then sees no GPU. C/C++ callers without torch are unaffected.
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        L = C.CDLL(SO_PATH)
        for name, (res, args) in list(SIGNATURES.items()) + list(SIGNATURES_GLOBAL_BA_SE3.items()) + list(SIGNATURES_TWO_VIEW.items()) \
                + list(SIGNATURES_SIM3.items()) + list(SIGNATURES_SIM3_MATCH.items()) + list(SIGNATURES_ESSENTIAL_GRAPH.items()) \
                + list(SIGNATURES_SEARCH_INIT.items()) + list(SIGNATURES_CULLING.items()) + list(SIGNATURES_RELOCALIZATION.items()) \
                + list(SIGNATURES_LOCAL_MAP.items()) + list(SIGNATURES_COVISIBILITY.items()) + list(SIGNATURES_MAP_CORRECTION.items()) \
                + list(SIGNATURES_KF_REMOVAL.items()) + list(SIGNATURES_MAP_FUSION.items()):
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc):
    if rc != VIORB_OK:
        raise ViorbError(rc, lib().viorb_last_error().decode())
    return rc


def ptr(a):
    """void* of a numpy array or a torch tensor (device or host)."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(C.c_void_p)
    return C.c_void_p(a.data_ptr())


def _torch_up(a, device=0):
    """A numpy array as a torch tensor on cuda:device (a structured dtype as its bytes)."""
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype.fields is not None:
        a = a.view(np.uint8)
    return torch.from_numpy(a).to(torch.device("cuda", device))


WORKSPACE_GUARD = 4096


class Workspace:
    """The one allocator of the caller workspaces the device entry points take: `nbytes` of device memory behind a 256-byte aligned
    pointer, with WORKSPACE_GUARD bytes behind them that no entry point may touch. fill: 0 (the default, what the wrappers always
    handed over), a byte value 1 .. 255, or None to leave the memory as the allocator returned it; the guard is filled with it too. The
    headers promise that a workspace's contents on entry are ignored, and tests/test_gpu_workspace_contents.py holds the library to
    that by re-filling `tensor` before a call and by handing one allocation to two problems of different sizes. A wrapper passes `ptr`
    and the byte count its own problem needs, never `nbytes`, which may be larger when an allocation is shared."""

    def __init__(self, torch, device, nbytes, fill=0):
        self.nbytes = int(nbytes)
        self.tensor = torch.empty(self.nbytes + 256 + WORKSPACE_GUARD, dtype=torch.uint8, device=device)
        self.offset = (-self.tensor.data_ptr()) % 256
        self.ptr = C.c_void_p(self.tensor.data_ptr() + self.offset)
        self.fill(fill)

    def fill(self, value):
        """Every byte of the allocation, guard included, set to `value`; None leaves it as it is."""
        if value is not None:
            self.tensor.fill_(int(value))
        return self

    def body(self, nbytes=None):
        """The first nbytes (default: all) of the workspace as a uint8 view."""
        n = self.nbytes if nbytes is None else int(nbytes)
        return self.tensor[self.offset:self.offset + n]

    def guard(self, nbytes=None):
        """The WORKSPACE_GUARD bytes behind a workspace of nbytes (default: all) as a uint8 view."""
        n = self.nbytes if nbytes is None else int(nbytes)
        assert n <= self.nbytes
        return self.tensor[self.offset + n:self.offset + n + WORKSPACE_GUARD]

    def fits(self, nbytes):
        return self.nbytes >= int(nbytes)
