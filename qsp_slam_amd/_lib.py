"""ctypes binding of libqsp_hip.so -- the C-ABI declared in include/qsp_hip.h.

There is NO CPU fallback: if the library is missing or no MI355X is visible the product path raises.  The oracle under
oracle/ is test infrastructure and is never imported from here.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("QSP_HIP_LIB", os.path.join(_HERE, "libqsp_hip.so"))   # override: experiments only

QSP_OK, QSP_ERR_INVALID, QSP_ERR_UNSUPPORTED, QSP_ERR_DEVICE, QSP_ERR_NO_DEVICE = 0, 1, 2, 3, 4

c_float_p = C.POINTER(C.c_float)
c_double_p = C.POINTER(C.c_double)
c_int32_p = C.POINTER(C.c_int32)
c_int64_p = C.POINTER(C.c_int64)
c_uint8_p = C.POINTER(C.c_uint8)


class QspError(RuntimeError):
    def __init__(self, code, msg):
        RuntimeError.__init__(self, "qsp_hip error %d: %s" % (code, msg))
        self.code = code


class DecoderDesc(C.Structure):
    _fields_ = [("n_layers", C.c_int32), ("code_len", C.c_int32), ("latent_in_layer", C.c_int32),
                ("in_dim", c_int32_p), ("out_dim", c_int32_p),
                ("weight", C.POINTER(c_float_p)), ("weight_g", C.POINTER(c_float_p)), ("bias", C.POINTER(c_float_p))]


class JointCfg(C.Structure):
    _fields_ = [("k1", C.c_float), ("k2", C.c_float), ("k3", C.c_float), ("k4", C.c_float),
                ("b1", C.c_float), ("b2", C.c_float), ("lr", C.c_float), ("s_damp", C.c_float),
                ("cut_off", C.c_float), ("n_iter", C.c_int32), ("n_depth", C.c_int32), ("code_len", C.c_int32)]


class RefineProfile(C.Structure):
    _fields_ = [("ms_total", C.c_float), ("ms_mlp_jtj", C.c_float), ("ms_mlp_fwd", C.c_float),
                ("ms_other", C.c_float), ("n_launch_jtj", C.c_int32), ("n_launch_fwd", C.c_int32),
                ("pts_jtj", C.c_int64), ("pts_fwd", C.c_int64), ("tiles_jtj", C.c_int64), ("tiles_fwd", C.c_int64),
                ("pts_band", C.c_int64), ("range_fallbacks", C.c_int32), ("screen_fallbacks", C.c_int32),
                ("screen_max_diff", C.c_float), ("screen_audit_failures", C.c_int32), ("pts_audit", C.c_int64)]


class BaScene(C.Structure):
    _fields_ = [("n_kf", C.c_int32), ("n_pt", C.c_int32), ("n_obj", C.c_int32), ("n_mono", C.c_int32),
                ("n_stereo", C.c_int32), ("n_objedge", C.c_int32),
                ("kf_pose", c_double_p), ("kf_fixed", c_uint8_p), ("kf_id", c_int64_p), ("kf_K", c_double_p),
                ("pt_xyz", c_double_p), ("pt_id", c_int64_p), ("obj_pose", c_double_p), ("obj_id", c_int64_p),
                ("mono_pt", c_int32_p), ("mono_kf", c_int32_p), ("mono_obs", c_double_p), ("mono_info", c_double_p),
                ("stereo_pt", c_int32_p), ("stereo_kf", c_int32_p), ("stereo_obs", c_double_p),
                ("stereo_info", c_double_p), ("objedge_kf", c_int32_p), ("objedge_obj", c_int32_p),
                ("objedge_meas", c_double_p), ("objedge_info", C.c_double)]


class BaTrace(C.Structure):
    _fields_ = [("cap", C.c_int32), ("n", C.c_int32), ("chi2", c_double_p), ("lam", c_double_p),
                ("trials", c_int32_p), ("accepted", c_int32_p), ("result", C.c_int32), ("iterations", C.c_int32),
                ("n_pose_blocks", C.c_int32), ("n_landmarks", C.c_int32)]


class BaProfile(C.Structure):
    _fields_ = [("ms_total", C.c_float), ("ms_linearize", C.c_float), ("ms_schur", C.c_float),
                ("ms_solve", C.c_float), ("ms_update", C.c_float), ("n_linearize", C.c_int32),
                ("n_trials", C.c_int32), ("bytes_linearize", C.c_int64), ("cholesky_chain", C.c_int32), ("chain_timeouts", C.c_int32),
                ("boundary_device", C.c_int32), ("boundary_host", C.c_int32), ("schur_form", C.c_int32)]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)   # qsp_allreduce_fn

_lib = None

# every symbol include/qsp_hip.h declares; tests/test_abi.py checks the list against the header
class PoseTrace(C.Structure):
    _fields_ = [("iters", C.c_int32 * 4), ("trace", C.c_double * 120)]


class Sim3Trace(C.Structure):
    _fields_ = [("iters", C.c_int32 * 2), ("trace", C.c_double * 60)]


class EssentialTrace(C.Structure):
    _fields_ = [("iters", C.c_int32), ("reserved", C.c_int32), ("trace", C.c_double * 128)]


class Detections(C.Structure):
    _fields_ = [("n_det", C.c_int32), ("T_cw", c_float_p), ("K", c_float_p), ("T_wo", c_float_p), ("code", c_float_p),
                ("n_flip", c_int32_p), ("flip_angle", C.c_double), ("pts_off", c_int32_p), ("pts_world", c_float_p),
                ("fg_off", c_int32_p), ("fg_px", c_float_p), ("fg_world", c_float_p), ("bg_off", c_int32_p),
                ("bg_rays", c_float_p)]


class DetectionResults(C.Structure):
    _fields_ = [("t_cam_obj", c_float_p), ("code", c_float_p), ("loss", c_float_p), ("is_good", c_uint8_p),
                ("kept_flip", c_int32_p), ("losses", c_float_p), ("pts_cam", c_float_p), ("rays", c_float_p),
                ("depth_obs", c_float_p), ("t_cam_obj_init", c_float_p)]


class ObjectGateIn(C.Structure):
    _fields_ = [("n_obj", C.c_int32), ("mode", c_int32_p), ("pts_off", c_int32_p), ("pts_world", c_float_p), ("T_wo", c_float_p),
                ("vert_off", c_int32_p), ("verts", c_float_p)]


class ObjectGateOut(C.Structure):
    _fields_ = [("erased", c_uint8_p), ("outlier", c_uint8_p), ("whl", c_float_p), ("R", c_float_p), ("centre_w", c_float_p),
                ("T_wo_pca", c_float_p), ("status", c_int32_p)]


class OrbFrame(C.Structure):
    _fields_ = [("n", C.c_int32), ("kp", c_float_p), ("octave", c_int32_p), ("desc", c_uint8_p),
                ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float),
                ("grid_cols", C.c_int32), ("grid_rows", C.c_int32), ("grid_w_inv", C.c_float), ("grid_h_inv", C.c_float),
                ("n_levels", C.c_int32), ("log_scale", C.c_float), ("scale_factors", c_float_p),
                ("Rcw", C.c_float * 9), ("tcw", C.c_float * 3),
                ("has_point", c_uint8_p), ("Xw", c_float_p), ("dist_min_inv", c_float_p), ("dist_max_inv", c_float_p),
                ("dist_max", c_float_p), ("mp_desc", c_uint8_p)]


class SearchSim3In(C.Structure):
    _fields_ = [("n_cand", C.c_int32), ("kf1", C.POINTER(OrbFrame)), ("kf2", C.POINTER(OrbFrame)), ("off2", c_int32_p),
                ("K", c_float_p), ("s12", c_float_p), ("R12", c_float_p), ("t12", c_float_p), ("th", c_float_p),
                ("pre1", c_uint8_p), ("pre2", c_uint8_p)]


class SearchSim3Out(C.Structure):
    _fields_ = [("match12", c_int32_p), ("n_found", c_int32_p), ("best1", c_int32_p), ("dist1", c_int32_p),
                ("best2", c_int32_p), ("dist2", c_int32_p)]


class BowFrame(C.Structure):
    _fields_ = [("n", C.c_int32), ("desc", c_uint8_p), ("angle", c_float_p), ("eligible", c_uint8_p), ("n_nodes", C.c_int32),
                ("node_id", c_int32_p), ("node_off", c_int32_p), ("feat", c_int32_p)]


class SearchBowIn(C.Structure):
    _fields_ = [("n_cand", C.c_int32), ("shared_is_source", C.c_int32), ("shared", C.POINTER(BowFrame)), ("cand", C.POINTER(BowFrame)),
                ("th", C.c_int32), ("th_inclusive", C.c_int32), ("nn_ratio", C.c_float), ("check_orientation", C.c_int32)]


class SearchBowOut(C.Structure):
    _fields_ = [("match", c_int32_p), ("n_matches", c_int32_p), ("match_raw", c_int32_p), ("dist", c_int32_p), ("hist", c_int32_p),
                ("ind", c_int32_p)]


class PlaceQueryIn(C.Structure):
    _fields_ = [("mode", C.c_int32), ("n", C.c_int32), ("word", c_int32_p), ("value", c_double_p), ("n_excluded", C.c_int32),
                ("excluded", c_int64_p), ("min_score", C.c_float), ("n_ref", C.c_int32), ("ref_id", c_int64_p)]


class PlaceQueryOut(C.Structure):
    _fields_ = [("n_sharing", C.c_int32), ("max_common", C.c_int32), ("min_common", C.c_int32), ("n_match", C.c_int32),
                ("min_score_used", C.c_float), ("match_id", c_int64_p), ("match_score", c_float_p), ("sharing_id", c_int64_p),
                ("sharing_common", c_int32_p), ("sharing_first", c_int32_p)]


class PlaceAccOut(C.Structure):
    _fields_ = [("n_cand", C.c_int32), ("cand_id", c_int64_p), ("acc_score", c_float_p), ("best_id", c_int64_p)]


class TriFrame(C.Structure):
    _fields_ = [("bow", BowFrame), ("xy", c_float_p), ("stereo", c_uint8_p), ("sigma2", c_float_p), ("scale", c_float_p)]


class SearchTriIn(C.Structure):
    _fields_ = [("n_cand", C.c_int32), ("kf1", C.POINTER(TriFrame)), ("kf2", C.POINTER(TriFrame)), ("F12", c_float_p), ("exy", c_float_p),
                ("th", C.c_int32), ("only_stereo", C.c_int32), ("check_orientation", C.c_int32)]


class SearchTriOut(C.Structure):
    _fields_ = SearchBowOut._fields_


class FuseIn(C.Structure):
    _fields_ = [("n_target", C.c_int32), ("target", C.POINTER(OrbFrame)), ("K", c_float_p), ("Ow", c_float_p), ("th", c_float_p),
                ("u_right_off", c_int32_p), ("u_right", c_float_p), ("inv_level_sigma2", c_float_p), ("check_reprojection", c_uint8_p),
                ("n_point", C.c_int32), ("Xw", c_float_p), ("normal", c_float_p), ("dist_min_inv", c_float_p), ("dist_max_inv", c_float_p),
                ("dist_max", c_float_p), ("desc", c_uint8_p), ("list_off", C.POINTER(C.c_int64)), ("list_idx", c_int32_p)]


class FuseOut(C.Structure):
    _fields_ = [("best_idx", c_int32_p), ("best_dist", c_int32_p), ("reason", c_int32_p), ("level", c_int32_p)]


class SearchProjIn(C.Structure):
    _fields_ = [("mode", C.c_int32), ("frame", C.POINTER(OrbFrame)), ("K", C.c_float * 5), ("Ow", C.c_float * 3), ("mb", C.c_float),
                ("u_right", c_float_p), ("slot_blocked", c_uint8_p), ("kp_angle", c_float_p),
                ("th", C.c_float), ("nn_ratio", C.c_float), ("view_cos_limit", C.c_float), ("check_orientation", C.c_int32), ("mono", C.c_int32),
                ("last_Rcw", C.c_float * 9), ("last_tcw", C.c_float * 3), ("n_src", C.c_int32),
                ("src_valid", c_uint8_p), ("src_blocks", c_uint8_p), ("Xw", c_float_p), ("desc", c_uint8_p), ("normal", c_float_p),
                ("dist_min_inv", c_float_p), ("dist_max_inv", c_float_p), ("dist_max", c_float_p), ("src_octave", c_int32_p), ("src_angle", c_float_p)]


class SearchProjOut(C.Structure):
    _fields_ = [("choice", c_int32_p), ("dist", c_int32_p), ("slot_src", c_int32_p), ("in_view", c_uint8_p), ("proj_x", c_float_p),
                ("proj_y", c_float_p), ("proj_xr", c_float_p), ("level", c_int32_p), ("view_cos", c_float_p), ("reason", c_int32_p),
                ("dist2", c_int32_p), ("level_best", c_int32_p), ("level2", c_int32_p), ("bin", c_int32_p), ("n_matches", C.c_int32),
                ("hist", C.c_int32 * 30), ("ind", C.c_int32 * 3), ("n_rounds", C.c_int32)]


class SearchProjKfIn(C.Structure):
    _fields_ = [("mode", C.c_int32), ("frame", C.POINTER(OrbFrame)), ("K", C.c_float * 4), ("Ow", C.c_float * 3),
                ("slot_blocked", c_uint8_p), ("kp_angle", c_float_p), ("th", C.c_float), ("orb_dist", C.c_int32),
                ("check_orientation", C.c_int32), ("n_src", C.c_int32), ("src_valid", c_uint8_p), ("Xw", c_float_p), ("desc", c_uint8_p),
                ("dist_min_inv", c_float_p), ("dist_max_inv", c_float_p), ("dist_max", c_float_p), ("normal", c_float_p),
                ("src_angle", c_float_p)]


class SearchProjKfOut(C.Structure):
    _fields_ = [("choice", c_int32_p), ("dist", c_int32_p), ("slot_src", c_int32_p), ("reason", c_int32_p), ("level", c_int32_p),
                ("proj_x", c_float_p), ("proj_y", c_float_p), ("bin", c_int32_p), ("n_matches", C.c_int32),
                ("hist", C.c_int32 * 30), ("ind", C.c_int32 * 3), ("n_rounds", C.c_int32)]


class TriangulateFrame(C.Structure):
    _fields_ = [("n", C.c_int32), ("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("Ow", C.c_float * 3),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("invfx", C.c_float), ("invfy", C.c_float),
                ("mb", C.c_float), ("mbf", C.c_float), ("xy_un", c_float_p), ("xy", c_float_p), ("u_right", c_float_p), ("depth", c_float_p),
                ("sigma2", c_float_p), ("scale", c_float_p)]


class TriangulateGeom(C.Structure):
    _fields_ = [("n_cand", C.c_int32), ("kf1", C.POINTER(TriangulateFrame)), ("kf2", C.POINTER(TriangulateFrame)), ("ratio_factor", C.c_float)]


class TriangulateOut(C.Structure):
    _fields_ = [("accept", c_uint8_p), ("first", c_uint8_p), ("x3D", c_float_p), ("n_new", c_int32_p), ("reason", c_int32_p), ("path", c_int32_p),
                ("cos_rays", c_float_p), ("z", c_float_p), ("err2", c_float_p), ("ratio_dist", c_float_p)]


SYMBOLS = [
    "qsp_last_error", "qsp_version", "qsp_device_count",
    "qsp_decoder_create", "qsp_decoder_destroy", "qsp_decoder_set_option", "qsp_decoder_get_counter", "qsp_decode_sdf",
    "qsp_decode_sdf_screen", "qsp_sdf_value_grad",
    "qsp_refine_batch_create", "qsp_refine_batch_destroy", "qsp_refine_batch_set_state", "qsp_refine_batch_run",
    "qsp_refine_batch_get", "qsp_refine_batch_trace", "qsp_refine_batch_trace_rot", "qsp_refine_batch_profile", "qsp_refine_batch_rows",
    "qsp_reconstruct_objects", "qsp_estimate_pose", "qsp_refine_detections",
    "qsp_decoder_group_create", "qsp_decoder_group_destroy", "qsp_refine_batch_create_group", "qsp_reconstruct_objects_group",
    "qsp_estimate_pose_group", "qsp_refine_detections_group",
    "qsp_mesh_extractor_create", "qsp_mesh_extractor_destroy", "qsp_mesh_extract", "qsp_mesh_from_volume", "qsp_mesh_fetch", "qsp_mesh_fetch_f64", "qsp_mesh_extractor_set_method",
    "qsp_mesh_extract_batch", "qsp_mesh_from_volumes", "qsp_mesh_fetch_batch", "qsp_mesh_extractor_set_batch_limit",
    "qsp_mesh_extractor_create_group", "qsp_mesh_extract_batch_group",
    "qsp_mc_tables",
    "qsp_pose_optimizer_create", "qsp_pose_optimizer_destroy", "qsp_pose_optimize", "qsp_ellipsoid_fit_planes", "qsp_ellipsoid_fit_prior",
    "qsp_sim3_optimize_batch", "qsp_sim3_ransac_batch", "qsp_search_by_sim3_batch", "qsp_search_by_bow_batch", "qsp_search_for_triangulation_batch", "qsp_fuse_batch", "qsp_search_by_projection", "qsp_search_by_projection_kf", "qsp_triangulate_batch", "qsp_create_new_map_points_batch", "qsp_essential_graph_optimize", "qsp_essential_graph_stages", "qsp_object_gates",
    "qsp_place_db_create", "qsp_place_db_destroy", "qsp_place_db_put", "qsp_place_db_list", "qsp_place_db_erase", "qsp_place_db_clear",
    "qsp_place_db_size", "qsp_place_db_query", "qsp_place_db_accumulate",
    "qsp_ba_create", "qsp_ba_destroy", "qsp_ba_set_levels", "qsp_ba_optimize", "qsp_ba_local_joint",
    "qsp_ba_set_state", "qsp_ba_get_state", "qsp_ba_get_edges", "qsp_ba_get_index", "qsp_ba_profile", "qsp_ba_set_shard", "qsp_ba_set_deterministic",
    "qsp_ba_set_shard_rccl", "qsp_ba_set_option", "qsp_ba_release_caches", "qsp_comm_unique_id", "qsp_comm_create", "qsp_comm_adopt", "qsp_comm_destroy", "qsp_comm_nccl", "qsp_comm_stub_counts",
    "qsp_comm_rank", "qsp_comm_world", "qsp_comm_allreduce_f64", "qsp_comm_allgather_f32",
]


def lib():
    """Loads the shared library once.  Raises if it was not built (python __graft_entry__.py / csrc/build.sh)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise QspError(QSP_ERR_NO_DEVICE, "libqsp_hip.so not built (%s); run qsp_slam_amd/csrc/build.sh -- there is "
                       "no CPU fallback" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    L.qsp_last_error.restype = C.c_char_p
    L.qsp_version.restype = C.c_int
    L.qsp_device_count.restype = C.c_int
    vp = C.c_void_p
    L.qsp_decoder_create.argtypes = [C.POINTER(DecoderDesc), C.c_int, C.POINTER(vp)]
    L.qsp_decoder_destroy.argtypes = [vp]
    L.qsp_decoder_set_option.argtypes = [vp, C.c_int32, C.c_int32]
    L.qsp_decoder_get_counter.argtypes = [vp, C.c_int32]
    L.qsp_decoder_get_counter.restype = C.c_int64
    L.qsp_decoder_destroy.restype = None
    L.qsp_decode_sdf.argtypes = [vp, c_float_p, c_float_p, C.c_int64, c_float_p]
    L.qsp_decode_sdf_screen.argtypes = [vp, c_float_p, c_float_p, C.c_int64, c_float_p]
    L.qsp_sdf_value_grad.argtypes = [vp, c_float_p, c_float_p, C.c_int64, c_float_p, c_float_p]
    pp_f = C.POINTER(c_float_p)
    L.qsp_refine_batch_create.argtypes = [vp, C.POINTER(JointCfg), C.c_int32, pp_f, c_int32_p, pp_f, c_int32_p, pp_f,
                                          c_int32_p, C.c_int32, c_int32_p, C.POINTER(vp)]
    L.qsp_refine_batch_destroy.argtypes = [vp]
    L.qsp_refine_batch_destroy.restype = None
    L.qsp_refine_batch_set_state.argtypes = [vp, c_float_p, c_float_p]
    L.qsp_refine_batch_run.argtypes = [vp, C.c_int32]
    L.qsp_refine_batch_get.argtypes = [vp, c_float_p, c_float_p, c_float_p, c_uint8_p]
    L.qsp_refine_batch_trace.argtypes = [vp, c_float_p, c_float_p, c_float_p, c_int32_p, c_int32_p, c_float_p]
    L.qsp_refine_batch_trace_rot.argtypes = [vp, c_float_p]
    L.qsp_refine_batch_profile.argtypes = [vp, C.c_int, C.POINTER(RefineProfile)]
    L.qsp_refine_batch_rows.argtypes = [vp, C.c_int, C.c_int32, c_float_p, c_float_p]
    L.qsp_reconstruct_objects.argtypes = [vp, C.POINTER(JointCfg), C.c_int32, pp_f, c_int32_p, pp_f, c_int32_p, pp_f,
                                          c_int32_p, C.c_int32, c_int32_p, c_float_p, c_float_p, c_float_p, c_float_p,
                                          c_float_p, c_uint8_p]
    L.qsp_estimate_pose.argtypes = [vp, C.c_int32, c_float_p, c_float_p, pp_f, c_int32_p, c_float_p, C.c_int32,
                                    c_float_p]
    L.qsp_refine_detections.argtypes = [vp, C.POINTER(JointCfg), C.POINTER(Detections), C.POINTER(DetectionResults)]
    L.qsp_decoder_group_create.argtypes = [C.POINTER(vp), C.c_int32, C.POINTER(vp)]
    L.qsp_decoder_group_destroy.argtypes = [vp]
    L.qsp_decoder_group_destroy.restype = None
    L.qsp_refine_batch_create_group.argtypes = [vp, C.POINTER(JointCfg), C.c_int32, pp_f, c_int32_p, pp_f, c_int32_p, pp_f,
                                                c_int32_p, c_int32_p, C.c_int32, c_int32_p, C.POINTER(vp)]
    L.qsp_reconstruct_objects_group.argtypes = [vp, C.POINTER(JointCfg), C.c_int32, pp_f, c_int32_p, pp_f, c_int32_p, pp_f,
                                                c_int32_p, c_int32_p, C.c_int32, c_int32_p, c_float_p, c_float_p, c_float_p,
                                                c_float_p, c_float_p, c_uint8_p]
    L.qsp_estimate_pose_group.argtypes = [vp, C.c_int32, c_float_p, c_float_p, pp_f, c_int32_p, c_float_p, c_int32_p, C.c_int32,
                                          c_float_p]
    L.qsp_refine_detections_group.argtypes = [vp, C.POINTER(JointCfg), C.POINTER(Detections), c_int32_p, C.POINTER(DetectionResults)]
    L.qsp_mesh_extractor_create.argtypes = [vp, C.c_int32, c_float_p, C.POINTER(vp)]
    L.qsp_mesh_extractor_destroy.argtypes = [vp]
    L.qsp_mesh_extractor_destroy.restype = None
    L.qsp_mesh_extract.argtypes = [vp, c_float_p, c_int64_p, c_int64_p]
    L.qsp_mesh_from_volume.argtypes = [vp, c_float_p, c_int64_p, c_int64_p]
    L.qsp_mesh_fetch.argtypes = [vp, c_float_p, c_int32_p, c_float_p]
    L.qsp_mesh_fetch_f64.argtypes = [vp, C.POINTER(C.c_double)]
    L.qsp_mesh_extractor_set_method.argtypes = [vp, C.c_int32]
    L.qsp_mesh_extract_batch.argtypes = [vp, C.c_int32, c_float_p, c_int64_p, c_int64_p]
    L.qsp_mesh_from_volumes.argtypes = [vp, C.c_int32, c_float_p, c_int64_p, c_int64_p]
    L.qsp_mesh_fetch_batch.argtypes = [vp, c_float_p, C.POINTER(C.c_double), c_int32_p, c_float_p]
    L.qsp_mesh_extractor_set_batch_limit.argtypes = [vp, C.c_int32]
    L.qsp_mesh_extractor_create_group.argtypes = [vp, C.c_int32, c_float_p, C.POINTER(vp)]
    L.qsp_mesh_extract_batch_group.argtypes = [vp, C.c_int32, c_float_p, c_int32_p, c_int64_p, c_int64_p]
    L.qsp_mc_tables.argtypes = [C.POINTER(C.c_int8), C.POINTER(C.c_int8)]
    L.qsp_pose_optimizer_create.argtypes = [C.c_int, C.c_int32, C.POINTER(vp)]
    L.qsp_pose_optimizer_destroy.argtypes = [vp]
    L.qsp_pose_optimizer_destroy.restype = None
    L.qsp_pose_optimize.argtypes = [vp, C.c_int32, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, c_uint8_p,
                                    c_double_p, c_uint8_p, c_int32_p, C.POINTER(PoseTrace)]
    L.qsp_ellipsoid_fit_planes.argtypes = [C.c_int, C.c_int32, c_double_p, c_int32_p, c_double_p, C.c_int32, C.c_int32,
                                           c_double_p, c_double_p, c_int32_p, c_double_p]
    L.qsp_ellipsoid_fit_prior.argtypes = [C.c_int, C.c_int32, c_double_p, c_int32_p, c_double_p, c_int32_p, c_double_p, c_double_p,
                                          c_double_p, c_double_p, C.c_double, C.c_int32, c_double_p, c_double_p, c_int32_p, c_double_p]
    L.qsp_sim3_optimize_batch.argtypes = [C.c_int, C.c_int32, c_int32_p] + [c_double_p] * 9 + [C.c_double, C.c_int32, c_double_p,
                                                                                                 c_uint8_p, c_int32_p, C.POINTER(Sim3Trace)]
    L.qsp_sim3_ransac_batch.argtypes = [C.c_int, C.c_int32] + [c_int32_p] * 4 + [c_float_p] * 6 + [C.c_int32, C.c_int32, c_int32_p,
                                                                                                    c_float_p, c_float_p, c_float_p,
                                                                                                    c_uint8_p, c_int32_p, c_int32_p]
    L.qsp_essential_graph_optimize.argtypes = [C.c_int, C.c_int32, c_double_p, c_uint8_p, C.c_int32, c_int32_p, c_int32_p, c_double_p,
                                               C.c_int32, C.c_int32, C.c_double, C.c_int32, c_double_p, c_int32_p, c_double_p,
                                               c_double_p, C.POINTER(EssentialTrace)]
    L.qsp_essential_graph_stages.argtypes = [C.c_int, C.c_int32, c_double_p, c_uint8_p, C.c_int32, c_int32_p, c_int32_p, c_double_p,
                                             C.c_int32, C.c_double] + [c_double_p] * 8
    L.qsp_search_by_sim3_batch.argtypes = [C.c_int, C.POINTER(SearchSim3In), C.POINTER(SearchSim3Out)]
    L.qsp_search_by_bow_batch.argtypes = [C.c_int, C.POINTER(SearchBowIn), C.POINTER(SearchBowOut)]
    L.qsp_search_for_triangulation_batch.argtypes = [C.c_int, C.POINTER(SearchTriIn), C.POINTER(SearchTriOut)]
    L.qsp_fuse_batch.argtypes = [C.c_int, C.POINTER(FuseIn), C.POINTER(FuseOut)]
    L.qsp_search_by_projection.argtypes = [C.c_int, C.POINTER(SearchProjIn), C.POINTER(SearchProjOut)]
    L.qsp_search_by_projection_kf.argtypes = [C.c_int, C.POINTER(SearchProjKfIn), C.POINTER(SearchProjKfOut)]
    L.qsp_triangulate_batch.argtypes = [C.c_int, C.POINTER(TriangulateGeom), c_int32_p, C.POINTER(TriangulateOut)]
    L.qsp_create_new_map_points_batch.argtypes = [C.c_int, C.POINTER(SearchTriIn), C.POINTER(TriangulateGeom), C.POINTER(SearchTriOut),
                                                  C.POINTER(TriangulateOut)]
    L.qsp_object_gates.argtypes = [C.c_int, C.POINTER(ObjectGateIn), C.POINTER(ObjectGateOut)]
    L.qsp_place_db_create.argtypes = [C.c_int, C.c_int64, C.c_int32, C.POINTER(vp)]
    L.qsp_place_db_destroy.argtypes = [vp]
    L.qsp_place_db_destroy.restype = None
    L.qsp_place_db_put.argtypes = [vp, C.c_int64, C.c_int32, c_int32_p, c_double_p, C.c_int32]
    L.qsp_place_db_list.argtypes = [vp, C.c_int64]
    L.qsp_place_db_erase.argtypes = [vp, C.c_int64]
    L.qsp_place_db_clear.argtypes = [vp]
    L.qsp_place_db_size.argtypes = [vp, c_int32_p, c_int32_p, c_int32_p, c_int64_p]
    L.qsp_place_db_query.argtypes = [vp, C.POINTER(PlaceQueryIn), C.POINTER(PlaceQueryOut)]
    L.qsp_place_db_accumulate.argtypes = [vp, C.c_int32, C.c_int32, c_int64_p, c_int32_p, c_int64_p, C.POINTER(PlaceAccOut)]
    L.qsp_ba_create.argtypes = [C.POINTER(BaScene), C.c_int, C.POINTER(vp)]
    L.qsp_ba_destroy.argtypes = [vp]
    L.qsp_ba_destroy.restype = None
    L.qsp_ba_set_levels.argtypes = [vp, c_uint8_p, c_uint8_p, c_uint8_p]
    L.qsp_ba_optimize.argtypes = [vp, C.c_int32, C.c_double, C.c_double, C.c_double, c_uint8_p, C.POINTER(BaTrace)]
    L.qsp_ba_local_joint.argtypes = [vp, c_uint8_p, C.POINTER(BaTrace), C.POINTER(BaTrace)]
    L.qsp_ba_set_state.argtypes = [vp, c_double_p, c_double_p, c_double_p]
    L.qsp_ba_get_state.argtypes = [vp, c_double_p, c_double_p, c_double_p]
    L.qsp_ba_get_edges.argtypes = [vp, c_double_p, c_double_p, c_double_p, c_uint8_p, c_uint8_p]
    L.qsp_ba_get_index.argtypes = [vp, c_int32_p, c_int32_p, c_int32_p]
    L.qsp_ba_profile.argtypes = [vp, C.c_int, C.POINTER(BaProfile)]
    L.qsp_ba_set_shard.argtypes = [vp, C.c_int32, C.c_int32, ALLREDUCE_FN, C.c_void_p]
    L.qsp_ba_set_deterministic.argtypes = [vp, C.c_int]
    L.qsp_ba_set_shard_rccl.argtypes = [vp, C.c_int32, C.c_int32, vp]
    L.qsp_ba_set_option.argtypes = [vp, C.c_int32, C.c_int32]
    L.qsp_comm_unique_id.argtypes = [c_uint8_p]
    L.qsp_comm_create.argtypes = [c_uint8_p, C.c_int32, C.c_int32, C.c_int, C.POINTER(vp)]
    L.qsp_comm_adopt.argtypes = [vp, C.c_int32, C.c_int32, C.c_int, C.POINTER(vp)]
    L.qsp_comm_destroy.argtypes = [vp]
    L.qsp_comm_destroy.restype = None
    L.qsp_comm_stub_counts.argtypes = [vp, c_int64_p]
    L.qsp_comm_nccl.argtypes = [vp]
    L.qsp_comm_nccl.restype = vp
    L.qsp_comm_rank.argtypes = [vp]
    L.qsp_comm_rank.restype = C.c_int32
    L.qsp_comm_world.argtypes = [vp]
    L.qsp_comm_world.restype = C.c_int32
    L.qsp_comm_allreduce_f64.argtypes = [vp, vp, C.c_int64, vp]
    L.qsp_comm_allgather_f32.argtypes = [vp, vp, vp, C.c_int64, vp]
    _lib = L
    return L


def check(rc):
    if rc != QSP_OK:
        raise QspError(rc, lib().qsp_last_error().decode("utf-8", "replace"))


def fptr(a):
    return a.ctypes.data_as(c_float_p)


def dptr(a):
    return a.ctypes.data_as(c_double_p)


def i32ptr(a):
    return a.ctypes.data_as(c_int32_p)


def i64ptr(a):
    return a.ctypes.data_as(c_int64_p)


def u8ptr(a):
    return a.ctypes.data_as(c_uint8_p)


def f32c(a):
    """C-contiguous float32 copy/view.  pybind11 hands Eigen::MatrixXf to Python as Fortran-ordered (M,3) arrays
    (src/LocalMapping_util.cc:705-706), so non-contiguous inputs are the normal case."""
    return np.ascontiguousarray(a, dtype=np.float32)


def ptr_array(arrs):
    """C array of float* over a list of contiguous float32 arrays (kept alive by the caller)."""
    t = c_float_p * len(arrs)
    return t(*[fptr(a) for a in arrs])
