"""The C ABI of include/dmvio_hip.h as ctypes sees it: pointer aliases, the mirrors of the header's structs, ONE signature table for every entry point (applied once, by
load_library), the loader, and what every wrapper module shares (error check, array-to-pointer helpers, the handle base).  tests/test_python_binding_cpu.py holds the table
and the mirrors against the header."""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libdmvio_hip.so")
INCLUDE_PATH = os.path.join(os.path.dirname(_HERE), "include", "dmvio_hip.h")

vp, ci, cf, cd, cz = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_size_t
c_f = C.POINTER(C.c_float)
c_d = C.POINTER(C.c_double)
c_i = C.POINTER(C.c_int)
c_u8 = C.POINTER(C.c_ubyte)
c_ll = C.POINTER(C.c_longlong)

_lib = None


class HipLibraryError(RuntimeError):
    pass


class TrackerSettings(C.Structure):
    """dmvio_hip_tracker_settings (settings.cpp:139-160)"""
    _fields_ = [("huberTH", cf), ("coarseCutoffTH", cf), ("affineOptModeA", cf), ("affineOptModeB", cf)]


_COARSE_UPDATE = C.CFUNCTYPE(ci, vp, c_d, c_d, cf, cf, c_d, c_d, c_d, c_d, c_d, c_d)
_COARSE_ACCEPT = C.CFUNCTYPE(None, vp)
_COARSE_VISUAL = C.CFUNCTYPE(None, vp, c_d, c_d, ci)


class CoarseCallbacks(C.Structure):
    """dmvio_hip_coarse_callbacks: the members of dmvio::IMUIntegration the coarse tracker calls."""
    _fields_ = [("user", vp), ("update", _COARSE_UPDATE), ("accept", _COARSE_ACCEPT), ("visual", _COARSE_VISUAL)]


_ALLREDUCE_F64 = C.CFUNCTYPE(ci, vp, c_d, cz)
_ALLGATHER = C.CFUNCTYPE(ci, vp, vp, vp, cz)


class CommCallbacks(C.Structure):
    """dmvio_hip_comm_callbacks (include/dmvio_hip.h): a caller-provided transport for the sharded BA iteration."""
    _fields_ = [("user", vp), ("allreduce_sum_f64", _ALLREDUCE_F64), ("allgather", _ALLGATHER)]


class BAFrameView(C.Structure):
    """dmvio_hip_ba_frame_view (include/dmvio_hip.h): what the BA hooks read of a keyframe."""
    _fields_ = [("frameID", ci), ("index", ci), ("PRE_worldToCam7", cd * 7), ("worldToCam_evalPT7", cd * 7), ("state10", cd * 10), ("state_zero10", cd * 10)]


_BA_COMPUTE = C.CFUNCTYPE(ci, vp, ci, c_d, c_d, cd, c_d, ci, C.POINTER(BAFrameView), c_d, c_d)
_BA_ACCEPT = C.CFUNCTYPE(None, vp, cd)
_BA_ENERGY = C.CFUNCTYPE(cd, vp, ci)
_BA_VALUES = C.CFUNCTYPE(None, vp, ci, C.POINTER(BAFrameView), c_d)
_BA_WEIGHT = C.CFUNCTYPE(cd, vp, cd, cd, ci)
_BA_BREAK = C.CFUNCTYPE(ci, vp)


class BACallbacks(C.Structure):
    """dmvio_hip_ba_callbacks: the members of dmvio::BAGTSAMIntegration the BA loop calls."""
    _fields_ = [("user", vp), ("computeBAUpdate", _BA_COMPUTE), ("acceptBAUpdate", _BA_ACCEPT), ("getBAEnergy", _BA_ENERGY), ("updateBAValues", _BA_VALUES),
                ("updateDynamicWeight", _BA_WEIGHT), ("canBreak", _BA_BREAK), ("postOptimization", _BA_VALUES)]


class BAVioOptions(C.Structure):
    _fields_ = [("coarseTrackingWasGood", ci), ("updateDynamicWeightDuringOptimization", ci), ("minOptIterations", ci), ("resInA_at_entry", ci),
                ("HMForGTSAM", c_d), ("bMForGTSAM", c_d)]


class PixelSelectorSettings(C.Structure):
    """dmvio_hip_pixel_selector_settings (settings.cpp:167-170)"""
    _fields_ = [("minGradHistCut", cf), ("minGradHistAdd", cf), ("gradDownweightPerLevel", cf), ("selectDirectionDistribution", ci)]


class PixelSelectorWindow(C.Structure):
    """dmvio_hip_pixel_selector_window (include/dmvio_hip.h): one window of a batched makeMaps call."""
    _fields_ = [("sel", vp), ("slot", ci), ("B_lut256", c_f), ("density", cf), ("recursions_left", ci), ("th_factor", cf),
                ("map_out_host", c_f), ("n_selected", ci), ("counts3", ci * 3)]


class NewTracesWindow(C.Structure):
    """dmvio_hip_new_traces_window: one window of dmvio_hip_immature_add_selected_batch."""
    _fields_ = [("imm", vp), ("host_tag", ci), ("host_slot", ci), ("sel", vp), ("first", ci)]


class TraceTablesWindow(C.Structure):
    """dmvio_hip_trace_tables_window (include/dmvio_hip.h): one window of dmvio_hip_immature_trace_batch."""
    _fields_ = [("imm", vp), ("new_slot", ci), ("n_hosts", ci), ("KRKi9", c_f), ("Kt3", c_f), ("aff2", c_f)]


class TraceWindow(C.Structure):
    """dmvio_hip_trace_window: one window of dmvio_hip_trace_new_coarse_batch."""
    _fields_ = [("imm", vp), ("new_slot", ci), ("new_w2c7", cd * 7), ("new_aff", cd * 2), ("new_exposure", cf), ("n_hosts", ci),
                ("host_c2w7", c_d), ("host_aff2", c_d), ("host_exposure", c_f), ("counts6", ci * 6)]


class ActivationWindow(C.Structure):
    """dmvio_hip_activation_window (include/dmvio_hip.h): one window of a batched activation call."""
    _fields_ = [("imm", vp), ("dm", vp), ("n_hosts", ci), ("KRKi9", c_f), ("Kt3", c_f), ("n_active", ci), ("active_host_tag", c_i),
                ("active_u", c_f), ("active_v", c_f), ("active_idepth", c_f), ("host_flagged", c_u8), ("newest_tag", ci), ("minActDist", cf),
                ("minTraceQuality", cf), ("n_selected", ci), ("n_deleted", ci)]


class BAMargWindow(C.Structure):
    """dmvio_hip_ba_marg_window: one window of dmvio_hip_ba_marginalize_points_batch."""
    _fields_ = [("ba", vp), ("candidates", vp), ("decision", vp), ("Hadd", vp), ("badd", vp), ("resInM", ci), ("update_prior", ci)]


class BAMargFrameWindow(C.Structure):
    """dmvio_hip_ba_marg_frame_window: one window of dmvio_hip_ba_marginalize_frame_batch."""
    _fields_ = [("ba", vp), ("frame", ci), ("HM_new", vp), ("bM_new", vp)]


class BAGraphWindow(C.Structure):
    """dmvio_hip_ba_graph_window: one window of dmvio_hip_ba_set_graph_from_batch."""
    _fields_ = [("ba", vp), ("graph", vp)]


class ActivationOptimize(C.Structure):
    """dmvio_hip_activation_optimize: one window of dmvio_hip_immature_optimize_selected_batch."""
    _fields_ = [("imm", vp), ("F", ci), ("frame_slots", c_i), ("w2c7", c_d), ("aff2", c_d), ("exposure", c_f), ("minObs", ci), ("result", c_i),
                ("idepth", c_f), ("res_state", c_i), ("n_activated", ci)]


class SetRefWindow(C.Structure):
    """dmvio_hip_set_ref_window (include/dmvio_hip.h): one window of dmvio_hip_tracker_set_ref_batch."""
    _fields_ = [("trk", vp), ("ref_slot", ci), ("ref_exposure", cf), ("ref_aff_a", cd), ("ref_aff_b", cd), ("n", ci), ("u", c_f), ("v", c_f), ("idepth", c_f), ("hdiF", c_f)]


class SetRefBaWindow(C.Structure):
    """dmvio_hip_set_ref_ba_window (include/dmvio_hip.h): one window of dmvio_hip_tracker_set_ref_from_ba_batch."""
    _fields_ = [("trk", vp), ("ba", vp), ("ref_slot", ci), ("ref_exposure", cf), ("ref_aff_a", cd), ("ref_aff_b", cd), ("n_selected", ci)]


class InitializerPointsWindow(C.Structure):
    """dmvio_hip_initializer_points_window (include/dmvio_hip.h): one window of dmvio_hip_initializer_set_points_batch."""
    _fields_ = [("ini", vp), ("n", ci), ("u", c_f), ("v", c_f), ("iR", c_f), ("isGood", c_u8), ("energy2", c_f), ("outlierTH", c_f)]


class InitializerWindow(C.Structure):
    """dmvio_hip_initializer_window (include/dmvio_hip.h): one window of dmvio_hip_initializer_calc_res_and_gs_batch."""
    _fields_ = [("ini", vp), ("lvl", ci), ("first_slot", ci), ("new_slot", ci), ("Ki9", cd * 9), ("fxfycxcy_lvl", cf * 4),
                ("refToNew7", cd * 7), ("aff_ab", cd * 2), ("idepth_new", c_f), ("alphaW", cf), ("alphaK", cf),
                ("couplingWeight", cf), ("priorY", cd), ("priorX", cd), ("H_out64", cf * 64), ("b_out8", cf * 8),
                ("H_sc64", cf * 64), ("b_sc8", cf * 8), ("res3", cf * 3), ("energy_new2", c_f), ("isGood_new", c_u8),
                ("maxstep", c_f), ("lastHessian_new", c_f), ("JbBuffer_new10", c_f)]


class InitializerLmWindow(C.Structure):
    """dmvio_hip_initializer_lm_window (include/dmvio_hip_init_lm_batch.h): one window of dmvio_hip_initializer_resident_track_frame_batch."""
    _fields_ = [("levels", C.POINTER(vp)), ("n_levels", ci), ("first_slot", ci), ("new_slot", ci), ("Ki9_levels", c_d), ("fxfycxcy_levels", c_f),
                ("alphaW", cf), ("alphaK", cf), ("regWeight", cf), ("couplingWeight", cf), ("priorY", cd), ("priorX", cd), ("wM8", c_f), ("fix_affine", ci),
                ("max_iterations", c_i), ("state_slot", ci), ("state_in10", c_d), ("state_out10", c_d), ("res3_levels", c_f), ("iterations_levels", c_i),
                ("trace_capacity", ci), ("trace_d", c_d), ("trace_f", c_f), ("trace_records", c_i), ("snapped", ci)]


# every `typedef struct` of the header that has a body -> its mirror
MIRRORS = {
    "dmvio_hip_tracker_settings": TrackerSettings, "dmvio_hip_coarse_callbacks": CoarseCallbacks, "dmvio_hip_set_ref_window": SetRefWindow,
    "dmvio_hip_set_ref_ba_window": SetRefBaWindow, "dmvio_hip_comm_callbacks": CommCallbacks, "dmvio_hip_ba_frame_view": BAFrameView,
    "dmvio_hip_ba_callbacks": BACallbacks, "dmvio_hip_ba_vio_options": BAVioOptions, "dmvio_hip_ba_marg_window": BAMargWindow,
    "dmvio_hip_ba_marg_frame_window": BAMargFrameWindow, "dmvio_hip_ba_graph_window": BAGraphWindow, "dmvio_hip_trace_tables_window": TraceTablesWindow,
    "dmvio_hip_trace_window": TraceWindow, "dmvio_hip_initializer_points_window": InitializerPointsWindow, "dmvio_hip_initializer_window": InitializerWindow,
    "dmvio_hip_pixel_selector_settings": PixelSelectorSettings, "dmvio_hip_pixel_selector_window": PixelSelectorWindow,
    "dmvio_hip_new_traces_window": NewTracesWindow, "dmvio_hip_activation_window": ActivationWindow, "dmvio_hip_activation_optimize": ActivationOptimize,
}

# entry point -> (restype, argtypes), in the header's order.  A handle is c_void_p; a pointer to one of the header's structs is POINTER(its mirror); an array the
# wrappers hand over as a plain address (numpy's .ctypes.data, a ctypes array, bytes) is c_void_p / c_char_p, every other one POINTER(its element type).
SIGNATURES = {
    "dmvio_hip_last_error": (C.c_char_p, []),
    "dmvio_hip_device_count": (ci, []),
    "dmvio_hip_create": (vp, [ci, ci, ci, ci]),
    "dmvio_hip_destroy": (None, [vp]),
    "dmvio_hip_pyr_levels": (ci, [vp]),
    "dmvio_hip_set_stream": (ci, [vp, vp]),
    "dmvio_hip_set_build_stream": (ci, [vp, vp]),
    "dmvio_hip_set_pyramid_tile_log2": (ci, [vp, ci]),
    "dmvio_hip_synchronize": (ci, [vp]),
    "dmvio_hip_frame_upload": (ci, [vp, ci, c_f]),
    "dmvio_hip_frame_from_device": (ci, [vp, ci, vp]),
    "dmvio_hip_undistorter_create": (vp, [vp, ci, ci, ci, c_f, c_f, c_f, c_f]),
    "dmvio_hip_undistorter_destroy": (None, [vp]),
    "dmvio_hip_frame_upload_raw": (ci, [vp, vp, ci, vp, cf, c_f]),
    "dmvio_hip_write_result_txt": (ci, [C.c_char_p, ci, vp, vp, vp, vp, vp, vp]),
    "dmvio_hip_frames_from_device_batch": (ci, [vp, ci, c_i, vp, cz]),
    "dmvio_hip_frames_attach_device_batch": (ci, [vp, ci, c_i, vp, cz]),
    "dmvio_hip_set_deferred_attach": (ci, [vp, ci]),
    "dmvio_hip_frames_from_raw_device_batch": (ci, [vp, vp, ci, c_i, vp, cz, cf]),
    "dmvio_hip_set_raw_batch_layout": (ci, [vp, ci]),
    "dmvio_hip_frame_level0_is_tiled": (ci, [vp, ci]),
    "dmvio_hip_set_raw_batch_kernel": (ci, [vp, ci]),
    "dmvio_hip_frame_mark_unclean": (ci, [vp, ci]),
    "dmvio_hip_frame_is_clean": (ci, [vp, ci]),
    "dmvio_hip_frame_download": (ci, [vp, ci, ci, c_f]),
    "dmvio_hip_frame_abs_squared_grad": (ci, [vp, ci, ci, c_f, C.POINTER(c_f)]),
    "dmvio_hip_tracker_create": (vp, [vp]),
    "dmvio_hip_tracker_destroy": (None, [vp]),
    "dmvio_hip_tracker_set_settings": (ci, [vp, C.POINTER(TrackerSettings)]),
    "dmvio_hip_tracker_make_k": (ci, [vp, c_f]),
    "dmvio_hip_tracker_set_ref": (ci, [vp, ci, cf, cd, cd, ci, c_f, c_f, c_f, c_f]),
    "dmvio_hip_tracker_pc_n": (ci, [vp, ci]),
    "dmvio_hip_tracker_get_pc": (ci, [vp, ci, c_f, c_f, c_f, c_f]),
    "dmvio_hip_tracker_get_idepth_map": (ci, [vp, ci, c_f, c_f]),
    "dmvio_hip_tracker_eval": (ci, [vp, ci, ci, cf, c_d, c_d, cf, c_d, c_d, c_d]),
    "dmvio_hip_tracker_track": (ci, [vp, ci, cf, c_d, c_d, ci, c_d, c_d, c_d, c_d, c_d, c_i]),
    "dmvio_hip_tracker_set_single_frame_mode": (ci, [vp, ci]),
    "dmvio_hip_tracker_set_launch_shape": (ci, [vp, ci, ci, ci, ci]),
    "dmvio_hip_tracker_set_eval_server": (ci, [vp, ci]),
    "dmvio_hip_tracker_set_batch_kernel": (ci, [vp, ci]),
    "dmvio_hip_tracker_set_residual_only_evals": (ci, [vp, ci]),
    "dmvio_hip_tracker_set_template_order": (ci, [vp, ci]),
    "dmvio_hip_tracker_debug_record_replay": (ci, [vp, ci]),
    "dmvio_hip_tracker_set_server_idle_us": (ci, [vp, ci]),
    "dmvio_hip_tracker_track_vio": (ci, [vp, ci, cf, c_d, c_d, ci, c_d, C.POINTER(CoarseCallbacks), c_d, c_d, c_d, c_d, c_i, c_i]),
    "dmvio_hip_coarse_update_visual": (ci, [C.POINTER(TrackerSettings), c_d, c_d, cf, cf, c_d, c_d, c_d, c_d, c_d]),
    "dmvio_hip_tracker_track_batch": (ci, [vp, ci, c_i, c_f, c_d, c_d, ci, c_d, c_d, c_d, c_d, c_d, c_i, c_i]),
    "dmvio_hip_tracker_track_batch_stage": (ci, [vp, ci, c_i, c_f, c_d, c_d, ci, c_d]),
    "dmvio_hip_tracker_track_batch_launch": (ci, [vp]),
    "dmvio_hip_tracker_track_batch_fetch_begin": (ci, [vp]),
    "dmvio_hip_tracker_track_batch_fetch": (ci, [vp, c_d, c_d, c_d, c_d, c_d, c_d, c_i, c_i]),
    "dmvio_hip_track_multi_create": (vp, [vp, ci, ci]),
    "dmvio_hip_track_multi_destroy": (None, [vp]),
    "dmvio_hip_tracker_track_multi": (ci, [vp, ci, C.POINTER(vp), ci, c_i, c_i, c_f, c_d, c_d, ci, c_d, c_d, c_d, c_d, c_d, c_i, c_i]),
    "dmvio_hip_track_multi_set_launch_shape": (ci, [vp, ci]),
    "dmvio_hip_track_multi_set_residual_only_evals": (ci, [vp, ci]),
    "dmvio_hip_track_multi_last_launch": (ci, [vp, c_i, c_i]),
    "dmvio_hip_track_multi_last_work": (ci, [vp, c_ll, c_ll]),
    "dmvio_hip_set_ref_batch_create": (vp, [vp, ci, ci]),
    "dmvio_hip_set_ref_batch_destroy": (None, [vp]),
    "dmvio_hip_tracker_set_ref_batch": (ci, [vp, ci, C.POINTER(SetRefWindow)]),
    "dmvio_hip_set_ref_batch_last_work": (ci, [vp, c_i, c_i, c_i, c_i]),
    "dmvio_hip_tracker_set_ref_from_ba": (ci, [vp, vp, ci, cf, cd, cd, c_i]),
    "dmvio_hip_tracker_set_ref_from_ba_batch": (ci, [vp, ci, C.POINTER(SetRefBaWindow)]),
    "dmvio_hip_make_track_hypotheses": (ci, [c_d, c_d, c_d, c_d, ci]),
    "dmvio_hip_tracker_track_new_coarse": (ci, [vp, ci, cf, ci, c_d, c_d, c_d, cd, c_d, c_d, c_d, c_i, c_i, c_i]),
    "dmvio_hip_tracker_last_work": (ci, [vp, c_ll, c_ll]),
    "dmvio_hip_tracker_last_residual_only_work": (ci, [vp, c_ll, c_ll]),
    "dmvio_hip_tracker_last_fused_builds": (ci, [vp]),
    "dmvio_hip_tracker_last_ticks": (ci, [vp, c_ll, c_ll]),
    "dmvio_hip_tracker_last_launch": (ci, [vp, c_i, c_i]),
    "dmvio_hip_selftest_divide": (ci, [vp, ci, vp, vp, vp, vp]),
    "dmvio_hip_ba_create": (vp, [vp]),
    "dmvio_hip_ba_destroy": (None, [vp]),
    "dmvio_hip_ba_set_stream": (ci, [vp, vp]),
    "dmvio_hip_ba_max_frames": (ci, []),
    "dmvio_hip_ba_set_window": (ci, [vp, ci, c_i, c_d, c_d, c_f, c_i, c_d]),
    "dmvio_hip_ba_set_marg_prior": (ci, [vp, c_d, c_d]),
    "dmvio_hip_ba_set_frame_state": (ci, [vp, ci, c_d]),
    "dmvio_hip_ba_set_frame_zero": (ci, [vp, ci, c_d]),
    "dmvio_hip_ba_set_frame_states": (ci, [vp, c_d, c_d]),
    "dmvio_hip_ba_set_frame_energy_th": (ci, [vp, c_f]),
    "dmvio_hip_ba_set_frame_energy_th_cap": (ci, [vp, cf]),
    "dmvio_hip_ba_set_calib_values": (ci, [vp, c_d, c_d]),
    "dmvio_hip_ba_marginalize_points": (ci, [vp, C.c_char_p, c_u8, c_d, c_d, c_i, ci]),
    "dmvio_hip_ba_marginalize_frame": (ci, [vp, ci, c_d, c_d]),
    "dmvio_hip_ba_get_marg_prior": (ci, [vp, c_d, c_d]),
    "dmvio_hip_ba_set_graph": (ci, [vp, ci, c_i, c_f, c_f, c_f, c_f, c_f, c_u8, ci, c_i, c_i]),
    "dmvio_hip_graph_create": (vp, []),
    "dmvio_hip_graph_destroy": (None, [vp]),
    "dmvio_hip_graph_clear": (ci, [vp]),
    "dmvio_hip_graph_insert_frame": (ci, [vp]),
    "dmvio_hip_graph_remove_frame": (ci, [vp, ci]),
    "dmvio_hip_graph_insert_point": (ci, [vp, ci, cf, cf, cf, c_f, c_f, ci]),
    "dmvio_hip_graph_remove_point": (ci, [vp, ci, ci]),
    "dmvio_hip_graph_insert_residual": (ci, [vp, ci, ci, ci]),
    "dmvio_hip_graph_drop_residual": (ci, [vp, ci, ci, ci]),
    "dmvio_hip_graph_set_residual_linearized": (ci, [vp, ci, ci, ci, c_f, c_f]),
    "dmvio_hip_graph_linearized_count": (ci, [vp]),
    "dmvio_hip_graph_export_linearized": (ci, [vp, c_u8, c_f, c_f]),
    "dmvio_hip_graph_set_idepth": (ci, [vp, ci, ci, cf]),
    "dmvio_hip_graph_set_idepths": (ci, [vp, ci, c_f]),
    "dmvio_hip_graph_counts": (ci, [vp, c_i, c_i, c_i]),
    "dmvio_hip_graph_frame_points": (ci, [vp, ci]),
    "dmvio_hip_graph_point_residuals": (ci, [vp, ci, ci]),
    "dmvio_hip_graph_export": (ci, [vp, c_i, c_f, c_f, c_f, c_f, c_f, c_u8, c_i, c_i]),
    "dmvio_hip_ba_set_graph_from": (ci, [vp, vp]),
    "dmvio_hip_ba_set_linearized_residuals": (ci, [vp, ci, vp, vp, vp, c_i]),
    "dmvio_hip_ba_get_linearized_residuals": (ci, [vp, ci, vp, vp, vp]),
    "dmvio_hip_ba_set_residual_flags": (ci, [vp, ci, vp]),
    "dmvio_hip_ba_fix_linearization": (ci, [vp, ci, vp, c_i]),
    "dmvio_hip_ba_get_lf_system": (ci, [vp, vp, vp]),
    "dmvio_hip_ba_activate_all": (ci, [vp]),
    "dmvio_hip_ba_linearize": (ci, [vp, ci, c_d]),
    "dmvio_hip_ba_apply": (ci, [vp]),
    "dmvio_hip_ba_get_res_state": (ci, [vp, c_u8, c_f, c_f, c_u8, c_f]),
    "dmvio_hip_ba_keep_jacobians": (ci, [vp, ci]),
    "dmvio_hip_ba_get_jacobians": (ci, [vp, c_f]),
    "dmvio_hip_ba_set_accumulators": (ci, [vp, ci]),
    "dmvio_hip_ba_get_frame_energy_th": (ci, [vp, c_f]),
    "dmvio_hip_ba_accumulate": (ci, [vp, c_d, c_d, c_d, c_d, c_i]),
    "dmvio_hip_ba_get_point_acc": (ci, [vp, c_f, c_f, c_f, c_f, c_f]),
    "dmvio_hip_ba_solve": (ci, [vp, ci, cd, c_d]),
    "dmvio_hip_ba_resubstitute": (ci, [vp, c_d]),
    "dmvio_hip_ba_get_points": (ci, [vp, c_f, c_f]),
    "dmvio_hip_ba_get_frame": (ci, [vp, ci, c_d, c_d, c_d]),
    "dmvio_hip_ba_get_calib": (ci, [vp, c_d]),
    "dmvio_hip_ba_get_calib_values": (ci, [vp, c_d, c_d]),
    "dmvio_hip_ba_get_res_in_a": (ci, [vp, c_i]),
    "dmvio_hip_ba_gn_iteration": (ci, [vp, ci, c_d, c_d, c_i]),
    "dmvio_hip_ba_profile_chain": (ci, [vp, ci, c_f]),
    "dmvio_hip_ba_last_decide_ticks": (ci, [vp, c_i]),
    "dmvio_hip_ba_set_comm": (ci, [vp, vp, ci, ci]),
    "dmvio_hip_ba_comm_timing": (ci, [vp, ci]),
    "dmvio_hip_ba_comm_times": (ci, [vp, vp, vp]),
    "dmvio_hip_ba_partition_points": (ci, [vp, ci, ci, cd, vp]),
    "dmvio_hip_ba_set_comm_callbacks": (ci, [vp, C.POINTER(CommCallbacks), ci, ci]),
    "dmvio_hip_tracker_set_comm": (ci, [vp, vp, ci, ci]),
    "dmvio_hip_tracker_set_comm_callbacks": (ci, [vp, C.POINTER(CommCallbacks), ci, ci]),
    "dmvio_hip_tracker_debug_split_single_rank": (ci, [vp, ci]),
    "dmvio_hip_comm_unique_id": (ci, [c_u8]),
    "dmvio_hip_comm_init_rank": (ci, [vp, c_u8, ci, ci, C.POINTER(vp)]),
    "dmvio_hip_comm_info": (ci, [vp, c_i, c_i]),
    "dmvio_hip_comm_destroy": (ci, [vp]),
    "dmvio_hip_ba_backup": (ci, [vp]),
    "dmvio_hip_ba_solve_system": (ci, [vp, ci, cd, c_d, c_d, c_d, c_d, c_d]),
    "dmvio_hip_ba_step": (ci, [vp, cf, c_f]),
    "dmvio_hip_ba_restore": (ci, [vp]),
    "dmvio_hip_ba_linearize_local": (ci, [vp, ci, c_d, c_f, c_i]),
    "dmvio_hip_ba_set_new_frame_energy_th": (ci, [vp, cf]),
    "dmvio_hip_ba_energy_terms": (ci, [vp, c_d, c_d]),
    "dmvio_hip_ba_optimize": (ci, [vp, ci, c_f, c_d, c_i, c_d]),
    "dmvio_hip_ba_optimize_vio": (ci, [vp, ci, C.POINTER(BACallbacks), C.POINTER(BAVioOptions), c_f, c_d, c_i, c_d]),
    "dmvio_hip_ba_batch_create": (vp, [vp, ci]),
    "dmvio_hip_ba_batch_destroy": (None, [vp]),
    "dmvio_hip_ba_optimize_batch": (ci, [vp, ci, vp, ci, vp, vp, vp, vp]),
    "dmvio_hip_ba_marginalize_points_batch": (ci, [vp, ci, C.POINTER(BAMargWindow)]),
    "dmvio_hip_ba_batch_last_marg_work": (ci, [vp, c_i, c_i, c_i, c_i]),
    "dmvio_hip_ba_batch_last_marg_ms": (ci, [vp, c_f]),
    "dmvio_hip_ba_marginalize_frame_batch": (ci, [vp, ci, C.POINTER(BAMargFrameWindow)]),
    "dmvio_hip_ba_batch_last_marg_frame_work": (ci, [vp, c_i, c_i, c_i, c_i]),
    "dmvio_hip_ba_batch_last_marg_frame_ms": (ci, [vp, c_f]),
    "dmvio_hip_ba_set_graph_from_batch": (ci, [vp, ci, C.POINTER(BAGraphWindow)]),
    "dmvio_hip_ba_batch_last_graph_work": (ci, [vp, c_i, c_i, c_i, c_i]),
    "dmvio_hip_ba_batch_last_graph_ms": (ci, [vp, c_f]),
    "dmvio_hip_ba_batch_set_exact_backsub": (ci, [vp, ci]),
    "dmvio_hip_ba_batch_last_ms": (ci, [vp, vp]),
    "dmvio_hip_ba_batch_set_profile": (ci, [vp, ci]),
    "dmvio_hip_ba_batch_set_streams": (ci, [vp, ci]),
    "dmvio_hip_ba_batch_set_linearize_lanes": (ci, [vp, ci]),
    "dmvio_hip_ba_batch_last_solve_ticks": (ci, [vp, vp]),
    "dmvio_hip_ba_batch_last_pivot_branch": (ci, [vp, ci, c_i]),
    "dmvio_hip_ba_batch_last_host_us": (ci, [vp, c_d]),
    "dmvio_hip_ba_debug_solve": (ci, [vp, ci, vp, vp, ci, vp, vp, vp, vp]),
    "dmvio_hip_ba_set_device_loop": (ci, [vp, ci]),
    "dmvio_hip_ba_get_last_x": (ci, [vp, vp]),
    "dmvio_hip_ba_solve_ldlt": (ci, [ci, c_d, c_d, c_d]),
    "dmvio_hip_ba_hook_ldlt": (ci, [vp, ci, c_d, c_d, cd, c_d, ci, C.POINTER(BAFrameView), c_d, c_d]),
    "dmvio_hip_ba_get_point_hessian": (ci, [vp, c_f]),
    "dmvio_hip_immature_create": (vp, [vp, ci]),
    "dmvio_hip_immature_destroy": (None, [vp]),
    "dmvio_hip_immature_clear": (ci, [vp]),
    "dmvio_hip_immature_count": (ci, [vp]),
    "dmvio_hip_immature_add_points": (ci, [vp, ci, ci, ci, c_i, c_i]),
    "dmvio_hip_immature_get_static": (ci, [vp, c_f, c_f, c_i, c_f, c_f, c_f, c_f]),
    "dmvio_hip_immature_get_state": (ci, [vp, c_f, c_f, c_f, c_f, c_f, c_i]),
    "dmvio_hip_immature_set_state": (ci, [vp, c_f, c_f, c_f, c_i]),
    "dmvio_hip_immature_trace": (ci, [vp, ci, ci, c_f, c_f, c_f]),
    "dmvio_hip_immature_optimize": (ci, [vp, ci, c_i, c_d, c_d, c_f, c_d, C.c_char_p, ci, c_i, c_f, c_i]),
    "dmvio_hip_trace_new_coarse": (ci, [vp, ci, c_d, c_d, cf, ci, c_d, c_d, c_f, c_d, c_i]),
    "dmvio_hip_trace_batch_create": (vp, [vp, ci]),
    "dmvio_hip_trace_batch_destroy": (None, [vp]),
    "dmvio_hip_immature_trace_batch": (ci, [vp, ci, C.POINTER(TraceTablesWindow)]),
    "dmvio_hip_trace_new_coarse_batch": (ci, [vp, ci, C.POINTER(TraceWindow), c_d, ci]),
    "dmvio_hip_initializer_create": (vp, [vp, ci]),
    "dmvio_hip_initializer_destroy": (None, [vp]),
    "dmvio_hip_initializer_set_points": (ci, [vp, ci, c_f, c_f, c_f, c_u8, c_f, c_f]),
    "dmvio_hip_initializer_calc_res_and_gs": (ci, [vp, ci, ci, ci, c_d, c_f, c_d, c_d, c_f, cf, cf, cf, cd, cd, c_f, c_f, c_f, c_f, c_f, c_f, c_u8, c_f, c_f, c_f]),
    "dmvio_hip_initializer_batch_create": (vp, [vp, ci]),
    "dmvio_hip_initializer_batch_destroy": (None, [vp]),
    "dmvio_hip_initializer_set_points_batch": (ci, [vp, ci, C.POINTER(InitializerPointsWindow)]),
    "dmvio_hip_initializer_calc_res_and_gs_batch": (ci, [vp, ci, C.POINTER(InitializerWindow)]),
    "dmvio_hip_initializer_batch_last_work": (ci, [vp, c_i, c_i, c_i, c_i]),
    "dmvio_hip_pixel_selector_default_settings": (None, [C.POINTER(PixelSelectorSettings)]),
    "dmvio_hip_pixel_selector_create": (vp, [vp, c_u8]),
    "dmvio_hip_pixel_selector_destroy": (None, [vp]),
    "dmvio_hip_pixel_selector_set_settings": (ci, [vp, C.POINTER(PixelSelectorSettings)]),
    "dmvio_hip_pixel_selector_get_potential": (ci, [vp]),
    "dmvio_hip_pixel_selector_set_potential": (ci, [vp, ci]),
    "dmvio_hip_pixel_selector_make_maps": (ci, [vp, ci, c_f, cf, ci, cf, c_i, c_i, c_f]),
    "dmvio_hip_pixel_selector_get_selection": (ci, [vp, c_i, c_i, c_i]),
    "dmvio_hip_pixel_selector_get_thresholds": (ci, [vp, c_f, c_f]),
    "dmvio_hip_pixel_selector_get_passes": (ci, [vp, ci, c_i, c_i]),
    "dmvio_hip_pixel_selector_get_stats": (ci, [vp, c_ll]),
    "dmvio_hip_immature_add_selected": (ci, [vp, ci, ci, vp]),
    "dmvio_hip_pixel_selector_batch_create": (vp, [vp, ci]),
    "dmvio_hip_pixel_selector_batch_destroy": (None, [vp]),
    "dmvio_hip_pixel_selector_make_maps_batch": (ci, [vp, ci, C.POINTER(PixelSelectorWindow)]),
    "dmvio_hip_immature_add_selected_batch": (ci, [vp, ci, C.POINTER(NewTracesWindow)]),
    "dmvio_hip_distance_map_create": (vp, [vp]),
    "dmvio_hip_distance_map_destroy": (None, [vp]),
    "dmvio_hip_distance_map_size": (ci, [vp, c_i, c_i]),
    "dmvio_hip_distance_map_tables_from_poses": (ci, [c_d, ci, c_d, c_d, c_f, c_f]),
    "dmvio_hip_distance_map_make": (ci, [vp, ci, c_f, c_f, ci, c_i, c_f, c_f, c_f]),
    "dmvio_hip_distance_map_add": (ci, [vp, ci, ci]),
    "dmvio_hip_distance_map_get": (ci, [vp, c_f]),
    "dmvio_hip_immature_set_types": (ci, [vp, c_f]),
    "dmvio_hip_immature_get_types": (ci, [vp, c_f]),
    "dmvio_hip_immature_set_last_trace": (ci, [vp, c_f, c_f]),
    "dmvio_hip_immature_select_for_activation": (ci, [vp, vp, ci, c_f, c_f, c_u8, ci, cf, cf, c_i, c_i]),
    "dmvio_hip_immature_get_activation_stats": (ci, [vp, c_ll]),
    "dmvio_hip_immature_get_activation": (ci, [vp, c_i, c_i]),
    "dmvio_hip_immature_get_marks": (ci, [vp, c_u8]),
    "dmvio_hip_immature_set_activation_walk": (ci, [vp, ci]),
    "dmvio_hip_immature_optimize_selected": (ci, [vp, ci, c_i, c_d, c_d, c_f, c_d, ci, c_i, c_f, c_i]),
    "dmvio_hip_immature_mark_optimized": (ci, [vp, c_i]),
    "dmvio_hip_immature_get_activated": (ci, [vp, c_i, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_i]),
    "dmvio_hip_immature_remove_marked": (ci, [vp]),
    "dmvio_hip_immature_remove_host": (ci, [vp, ci]),
    "dmvio_hip_min_act_dist_update": (cf, [cf, ci, cf]),
    "dmvio_hip_activation_batch_create": (vp, [vp, ci]),
    "dmvio_hip_activation_batch_destroy": (None, [vp]),
    "dmvio_hip_distance_map_make_batch": (ci, [vp, ci, C.POINTER(ActivationWindow)]),
    "dmvio_hip_immature_select_for_activation_batch": (ci, [vp, ci, C.POINTER(ActivationWindow)]),
    "dmvio_hip_immature_optimize_selected_batch": (ci, [vp, ci, C.POINTER(ActivationOptimize), c_d]),
    "dmvio_hip_immature_remove_marked_batch": (ci, [vp, ci, C.POINTER(vp), c_i]),
}

# The same for the extension headers beside include/dmvio_hip.h, header by header, under the same rules: the table above is held to that header alone, entry for entry.
EXTENSION_SIGNATURES = {
    "dmvio_hip_init_resident.h": {
        "dmvio_hip_initializer_set_resident": (ci, [vp, ci, c_f, c_f, c_f, c_f, c_u8, c_f, c_f, c_f, c_i, c_i]),
        "dmvio_hip_initializer_resident_reset_unsnapped": (ci, [vp]),
        "dmvio_hip_initializer_resident_reset_points": (ci, [vp, ci]),
        "dmvio_hip_initializer_resident_do_step": (ci, [vp, cf, c_f]),
        "dmvio_hip_initializer_resident_apply_step": (ci, [vp]),
        "dmvio_hip_initializer_resident_opt_reg": (ci, [vp, cf]),
        "dmvio_hip_initializer_resident_propagate_down": (ci, [vp, vp, cf, ci]),
        "dmvio_hip_initializer_resident_propagate_up": (ci, [vp, vp, cf, ci]),
        "dmvio_hip_initializer_resident_calc": (ci, [vp, ci, ci, ci, c_d, c_f, c_d, c_d, cf, cf, cf, cd, cd, ci, c_f, c_f, c_f, c_f, c_f, c_f]),
        "dmvio_hip_initializer_resident_get_state": (ci, [vp, c_f, c_f, c_u8, c_f, c_f, c_f, c_u8, c_f, c_f, c_f, c_f]),
        "dmvio_hip_initializer_resident_set_state": (ci, [vp, c_f, c_f, c_u8, c_f, c_f, c_f, c_u8, c_f, c_f, c_f, c_f, c_f]),
        "dmvio_hip_initializer_resident_last_work": (ci, [vp, c_i, c_i, c_i, c_i]),
    },
    "dmvio_hip_init_lm.h": {
        "dmvio_hip_initializer_lm_control_host": (ci, [c_f, c_f, c_f, c_f, cf, ci, c_f, ci, c_d, c_d, c_f, c_d, c_d, c_d]),
        "dmvio_hip_initializer_debug_lm_control": (ci, [vp, c_f, c_f, c_f, c_f, cf, ci, c_f, ci, c_d, c_d, c_f, c_d, c_d, c_d]),
        "dmvio_hip_initializer_resident_track_level": (ci, [vp, ci, ci, ci, c_d, c_f, cf, cf, cf, cf, cd, cd, c_f, ci, ci, ci, c_d, c_d, c_f, c_i, ci, c_d, c_f, c_i]),
        "dmvio_hip_initializer_resident_track_frame": (ci, [C.POINTER(vp), ci, ci, ci, c_d, c_f, cf, cf, cf, cf, cd, cd, c_f, ci, c_i, c_d, c_d, c_f, c_i, ci, c_d, c_f, c_i]),
        "dmvio_hip_initializer_lm_last_work": (ci, [vp, c_i, c_i, c_i, c_i]),
    },
    "dmvio_hip_init_lm_batch.h": {
        "dmvio_hip_initializer_lm_batch_create": (vp, [vp, ci]),
        "dmvio_hip_initializer_lm_batch_destroy": (None, [vp]),
        "dmvio_hip_initializer_resident_track_frame_batch": (ci, [vp, ci, C.POINTER(InitializerLmWindow)]),
        "dmvio_hip_initializer_lm_batch_last_work": (ci, [vp, c_i, c_i, c_i, c_i]),
    },
    "dmvio_hip_init_first.h": {
        "dmvio_hip_init_first_create": (vp, [vp]),
        "dmvio_hip_init_first_destroy": (None, [vp]),
        "dmvio_hip_init_first_make_pixel_status": (ci, [vp, ci, ci, cf, ci, cf, c_i, c_i, c_u8]),
        "dmvio_hip_init_first_get_passes": (ci, [vp, ci, c_i, c_f, c_i]),
        "dmvio_hip_init_first_make_nn": (ci, [vp, ci, c_f, c_f, ci, c_f, c_f, c_i, c_i]),
        "dmvio_hip_initializer_set_first": (ci, [vp, vp, ci, c_f, ci, C.POINTER(vp), c_f, cf, c_i, c_i]),
        "dmvio_hip_init_first_get_level": (ci, [vp, ci, c_f, c_f, c_f, c_i, c_i]),
        "dmvio_hip_init_first_last_work": (ci, [vp, c_i, c_i, c_i, c_i]),
    },
}
# the structs of the extension headers -> their mirrors, header by header (MIRRORS is held to include/dmvio_hip.h alone)
EXTENSION_MIRRORS = {
    "dmvio_hip_init_lm_batch.h": {"dmvio_hip_initializer_lm_window": InitializerLmWindow},
}


def all_signatures():
    """every entry point of the library the package knows: the main header's table, then the extension headers'"""
    out = dict(SIGNATURES)
    for table in EXTENSION_SIGNATURES.values():
        out.update(table)
    return out


def apply_signatures(L, allow_missing=False):
    for name, (restype, argtypes) in all_signatures().items():
        try:
            fn = getattr(L, name)
        except AttributeError:
            if allow_missing:
                continue
            raise HipLibraryError("%s lacks %s, which include/dmvio_hip.h declares" % (getattr(L, "_name", "the library"), name))
        fn.restype, fn.argtypes = restype, argtypes
    return L


def load_library(path=None, allow_missing=False):
    """dlopen libdmvio_hip.so and give every entry point its signature, once.  Raises HipLibraryError when it has not been built — never falls back.
    path: another build of the library; it replaces the tree's as the library every later call without a path returns (a tool timing a parent build loads it first).
    allow_missing: skip the table entries such a build does not export yet; by default a missing entry point raises."""
    global _lib
    if _lib is None or path is not None:
        path = path or LIB_PATH
        if not os.path.exists(path):
            raise HipLibraryError("libdmvio_hip.so not built (%s); run `python -c 'import __graft_entry__ as g; g.build()'`" % path)
        # torch wheels bundle their own libamdhip64; when torch shares the process (bench.py uses it for device
        # memory, streams and RCCL) it must be loaded FIRST so that both sides run on one HIP runtime — two
        # runtimes in one process leave the second one without devices ("No HIP GPUs are available").
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        _lib = apply_signatures(C.CDLL(path), allow_missing)
    return _lib


def declared_symbols():
    """Entry points declared in include/dmvio_hip.h (parsed from the header text)."""
    txt = open(INCLUDE_PATH).read()
    return sorted(set(re.findall(r"\b(dmvio_hip_[a-z0-9_]+)\s*\(", txt)))


def _err(L):
    return (L.dmvio_hip_last_error() or b"").decode()


def _chk(L, r, what):
    if r is None or (isinstance(r, int) and r < 0):
        raise HipLibraryError("%s: %s" % (what, _err(L)))
    return r


def _f(a):
    return a.ctypes.data_as(c_f)


def _d(a):
    return a.ctypes.data_as(c_d)


def _i(a):
    return a.ctypes.data_as(c_i)


def _u8(a):
    return a.ctypes.data_as(c_u8)


class _Handle:
    """One object of the library behind an opaque pointer: the library L, the pointer p and the name of the entry point that destroys it."""
    _destroy = None

    def _create(self, L, create, *args, what=None):
        self.L = L
        p = getattr(L, create)(*args)
        if not p:
            raise HipLibraryError("%s: %s" % (what or create, _err(L)))
        self.p = C.c_void_p(p)

    def close(self):
        p, self.p = getattr(self, "p", None), None
        if p:
            getattr(self.L, self._destroy)(p)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _outs(self, name, ctype, n, *args):
        """dmvio_hip_<name>(p, *args, &out[0] .. &out[n-1]) for n out-parameters of one C type -> the n values"""
        out = [ctype() for _ in range(n)]
        _chk(self.L, getattr(self.L, "dmvio_hip_" + name)(self.p, *args, *[C.byref(x) for x in out]), name)
        return tuple(x.value for x in out)
