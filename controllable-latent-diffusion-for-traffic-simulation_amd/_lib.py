"""ctypes binding of libcld_hip.so (C-ABI: include/cld.h, include/cld_lane.h, include/cld_recon.h, include/cld_solver.h,
include/cld_eval.h).

The product path has NO fallback: if the HIP library is missing or a call
fails, a `CldError` is raised.  Nothing under `oracle/` is ever imported here.
"""
from __future__ import annotations

import ctypes as C
import os

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# CLD_LIB_PATH selects an experimental build of the same library (never a different backend)
LIB_PATH = os.environ.get("CLD_LIB_PATH") or os.path.join(PKG_DIR, "libcld_hip.so")


class CldError(RuntimeError):
    pass


class CldConfig(C.Structure):
    _fields_ = [
        ("horizon", C.c_int32), ("latent_dim", C.c_int32), ("cond_dim", C.c_int32), ("base_dim", C.c_int32),
        ("dim_mults", C.c_int32 * 3), ("hidden", C.c_int32), ("n_timesteps", C.c_int32),
        ("step_time", C.c_float), ("acce_bound", C.c_float * 2), ("v_bound", C.c_float * 2),
        ("max_steer", C.c_float), ("max_yawvel", C.c_float),
        ("norm_mean", C.c_float * 6), ("norm_std", C.c_float * 6),
        ("precision", C.c_int32),
    ]


PRECISIONS = {"f32": 0, "f16x2": 1}
OPTIMIZERS = {"adam": 0, "sgd": 1}
RES_FOLD = {"fused": 0, "separate": 1}      # cld_debug_res_fold (include/cld.h CLD_RES_FOLD_*)
KERNELS = {"guide": 0, "decode": 1, "encode": 2, "unet": 3, "context": 4, "conv5": 5}        # cld_debug_force_kernel
# cld_debug_force_kernel: the formulations each kernel has (include/cld.h CLD_FORM_*).  The numbers are reused across kernels (3 is "quad"
# for the guide kernel, "chain1" for the U-Net and "winograd_whole" for the k5 layers), so a form
# is named together with its kernel: form_id() refuses a name the kernel does not have.
KERNEL_FORMS = {
    "guide": {"auto": 0, "valu": 1, "mfma": 2, "quad": 3},
    "decode": {"auto": 0, "valu": 1, "mfma": 2},
    "encode": {"auto": 0, "valu": 1, "mfma": 2},
    "unet": {"auto": 0, "layers": 1, "chain": 2, "chain1": 3, "chain4": 4, "chainw": 5, "chainw2": 6, "chainw1": 7},      # one launch per layer / LDS-resident layer chains
    "context": {"auto": 0, "direct": 1, "winograd": 2},       # the 3x3 / stride-1 convolutions of the ResNet-18
    "conv5": {"auto": 0, "direct": 1, "winograd": 2, "winograd_whole": 3, "winograd_ksplit": 4},     # the k5 layers of the U-Net's L = 13 / 26 levels
}
FORMS = {name: v for forms in KERNEL_FORMS.values() for name, v in forms.items()}      # every name -> its number (the union of the above)


def form_id(kind: str, name: str) -> int:
    """The CLD_FORM_* number of formulation `name` of kernel `kind`; raises ValueError on a kernel or a name that kernel does not have."""
    if kind not in KERNEL_FORMS:
        raise ValueError(f"unknown kernel '{kind}' (one of {sorted(KERNEL_FORMS)})")
    forms = KERNEL_FORMS[kind]
    if name not in forms:
        raise ValueError(f"kernel '{kind}' has no formulation '{name}' (one of {sorted(forms)})")
    return forms[name]


class CldGuidance(C.Structure):
    """include/cld.h `cld_guidance` (device pointers + optimiser settings of the sampling-time guidance step)."""
    _fields_ = [("curr_states", C.c_void_p), ("target_speed", C.c_void_p), ("loss_scale", C.c_void_p),
                ("lr", C.c_float), ("perturb_th", C.c_float), ("optimizer", C.c_int32),
                ("speed_limit", C.c_float), ("acc_limit", C.c_float),
                ("speed_limit_scale", C.c_void_p), ("acc_limit_scale", C.c_void_p),
                ("target_pos", C.c_void_p), ("target_time", C.c_void_p), ("target_pos_scale", C.c_void_p),
                ("ext_grad", C.c_void_p),
                ("apply_output", C.c_int32), ("no_intermediate", C.c_int32),
                ("final_lr", C.c_float), ("final_perturb_th", C.c_float), ("final_optimizer", C.c_int32),
                ("grad_steps", C.c_int32), ("final_grad_steps", C.c_int32), ("guide_clean", C.c_int32),
                ("collision", C.c_void_p),        # const cld_collision*
                ("map_collision", C.c_void_p)]    # const cld_map_collision*


class CldCollision(C.Structure):
    """include/cld.h `cld_collision` (upstream's AgentCollisionLoss configured per scene, device pointers)."""
    _fields_ = [("extent", C.c_void_p), ("world_from_agent", C.c_void_p), ("curr_speed", C.c_void_p),
                ("scene_start", C.c_void_p), ("scene_weight", C.c_void_p), ("guided", C.c_void_p),
                ("num_scenes", C.c_int32), ("num_samp", C.c_int32), ("num_disks", C.c_int32), ("max_scene_agents", C.c_int32),
                ("buffer_dist", C.c_float), ("decay_rate", C.c_float), ("moving_speed_th", C.c_float), ("excluded", C.c_void_p)]


class CldMapCollision(C.Structure):
    """include/cld.h `cld_map_collision` (upstream's MapCollisionLoss configured per scene, device pointers)."""
    _fields_ = [("extent", C.c_void_p), ("raster_from_agent", C.c_void_p), ("drivable_map", C.c_void_p), ("curr_speed", C.c_void_p),
                ("scene_start", C.c_void_p), ("scene_weight", C.c_void_p),
                ("num_scenes", C.c_int32), ("num_samp", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("num_points_l", C.c_int32), ("num_points_w", C.c_int32), ("decay_rate", C.c_float), ("moving_speed_th", C.c_float)]


class CldMapSource(C.Structure):
    """include/cld.h `cld_map_source` (the scene maps a map_collision term without a drivable_map reads, device pointers)."""
    _fields_ = [("maps", C.c_void_p), ("scene_map", C.c_void_p), ("map_from_world", C.c_void_p), ("world", C.c_void_p),
                ("num_scenes", C.c_int32), ("num_maps", C.c_int32), ("n_sem", C.c_int32), ("map_h", C.c_int32), ("map_w", C.c_int32),
                ("drivable_layer", C.c_int32), ("px_per_m", C.c_float), ("ego_center", C.c_float * 2), ("no_map_fill", C.c_float)]


class CldGoal(C.Structure):
    """include/cld.h `cld_goal` (upstream's GlobalTargetPosLoss / GlobalTargetPosAtTimeLoss per agent, device pointers)."""
    _fields_ = [("target_pos", C.c_void_p), ("agent_from_world", C.c_void_p), ("kind", C.c_void_p), ("target_time", C.c_void_p),
                ("urgency", C.c_void_p), ("pref_speed", C.c_void_p), ("scale", C.c_void_p), ("reached", C.c_void_p),
                ("num_samp", C.c_int32), ("global_t", C.c_int32), ("dt", C.c_float), ("min_progress_dist", C.c_float)]


class CldSocialGroup(C.Structure):
    """include/cld.h `cld_social_group` (upstream's SocialGroupLoss over all groups of a batch, device pointers)."""
    _fields_ = [("group_start", C.c_void_p), ("member", C.c_void_p), ("leader", C.c_void_p), ("social_dist", C.c_void_p),
                ("cohesion", C.c_void_p), ("scale", C.c_void_p), ("world_from_agent", C.c_void_p), ("draw_r", C.c_void_p),
                ("draw_u", C.c_void_p), ("seed", C.c_uint64), ("num_groups", C.c_int32), ("num_samp", C.c_int32),
                ("max_members", C.c_int32), ("iter_base", C.c_int32), ("n_iter", C.c_int32), ("n_opt", C.c_int32)]


SOCIAL_MAX_MEMBERS = 128               # include/cld.h: the bound on cld_social_group.max_members


class CldPairTerm(C.Structure):
    """include/cld.h `cld_pair_term` (upstream's pair-relation losses over all pairs of a batch, device pointers)."""
    _fields_ = [("target", C.c_void_p), ("ref", C.c_void_p), ("kind", C.c_void_p), ("lo", C.c_void_p), ("hi", C.c_void_p),
                ("decay", C.c_void_p), ("scale", C.c_void_p), ("world_from_agent", C.c_void_p), ("agent_from_world", C.c_void_p),
                ("agent_start", C.c_void_p), ("agent_id", C.c_void_p), ("incidence", C.c_void_p), ("num_pairs", C.c_int32),
                ("num_samp", C.c_int32), ("num_involved", C.c_int32), ("num_incidences", C.c_int32)]


# include/cld.h CLD_PAIR_*: the relation a pair term evaluates
PAIR_KINDS = {"keep_distance": 0, "collision": 1, "stay_away": 2, "front_collision": 3, "collide_left": 4}


class CldLaneTerm(C.Structure):
    """include/cld_lane.h `cld_lane_term` (upstream's lane-projection losses over the entries of a batch, device pointers)."""
    _fields_ = [("lines", C.c_void_p), ("agent", C.c_void_p), ("line", C.c_void_p), ("kind", C.c_void_p), ("decay", C.c_void_p),
                ("scale", C.c_void_p), ("num_entries", C.c_int32), ("num_lines", C.c_int32), ("max_pts", C.c_int32), ("num_samp", C.c_int32)]


# include/cld_lane.h CLD_LANE_*: the loss a lane entry evaluates
LANE_KINDS = {"following": 0, "change_left": 1, "follow_decayed": 2}
LANE_MAX_PTS = 1024                    # include/cld_lane.h CLD_LANE_MAX_PTS


class CldRaster(C.Structure):
    """include/cld.h `cld_raster` (the scene an observation raster is built from, device pointers)."""
    _fields_ = [("hist_world", C.c_void_p), ("hist_avail", C.c_void_p), ("scene_start", C.c_void_p), ("maps", C.c_void_p),
                ("scene_map", C.c_void_p), ("map_from_world", C.c_void_p),
                ("num_scenes", C.c_int32), ("B_all", C.c_int32), ("T_hist", C.c_int32), ("n_sem", C.c_int32), ("height", C.c_int32),
                ("width", C.c_int32), ("num_maps", C.c_int32), ("map_h", C.c_int32), ("map_w", C.c_int32),
                ("px_per_m", C.c_float), ("ego_center", C.c_float * 2), ("no_map_fill", C.c_float), ("max_neighbor_dist", C.c_float)]


class CldSceneMetrics(C.Structure):
    """include/cld.h `cld_scene_metrics` (the scene set the closed-loop episode metrics are computed over, device pointers)."""
    _fields_ = [("extent", C.c_void_p), ("scene_start", C.c_void_p), ("maps", C.c_void_p), ("scene_map", C.c_void_p),
                ("map_from_world", C.c_void_p), ("sim_dt", C.c_double), ("stat_dt", C.c_double),
                ("num_scenes", C.c_int32), ("B_all", C.c_int32), ("n_sem", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("num_maps", C.c_int32), ("map_h", C.c_int32), ("map_w", C.c_int32), ("drivable_layer", C.c_int32),
                ("px_per_m", C.c_float), ("ego_center", C.c_float * 2), ("no_map_fill", C.c_float)]


class CldGuideMetrics(C.Structure):
    """include/cld.h `cld_guide_metrics` (the scene set and the entry table the guidance satisfaction metrics are computed over, device
    pointers)."""
    _fields_ = [("extent", C.c_void_p), ("scene_start", C.c_void_p), ("maps", C.c_void_p), ("scene_map", C.c_void_p),
                ("map_from_world", C.c_void_p), ("entry_kind", C.c_void_p), ("entry_scene", C.c_void_p), ("member_start", C.c_void_p),
                ("members", C.c_void_p), ("excl_start", C.c_void_p), ("excluded", C.c_void_p), ("param_start", C.c_void_p),
                ("params", C.c_void_p),
                ("num_entries", C.c_int32), ("num_members", C.c_int32), ("num_excluded", C.c_int32), ("num_params", C.c_int32),
                ("num_scenes", C.c_int32), ("B_all", C.c_int32), ("n_sem", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("num_maps", C.c_int32), ("map_h", C.c_int32), ("map_w", C.c_int32), ("drivable_layer", C.c_int32),
                ("px_per_m", C.c_float), ("ego_center", C.c_float * 2), ("no_map_fill", C.c_float)]


# cld_guide_metrics.entry_kind (include/cld.h CLD_GM_*), under upstream's metric names
GUIDE_METRIC_KINDS = {"target_speed": 0, "speed_limit": 1, "acc_limit": 2, "agent_collision": 3, "agent_collision_disk": 4, "social_dist": 5,
                      "map_collision": 6, "map_collision_disk": 7, "target_pos": 8, "global_target_pos": 9, "target_pos_at_time": 10,
                      "global_target_pos_at_time": 11, "social_group": 12}


class CldOccupancy(C.Structure):
    """include/cld.h `cld_occupancy` (one occupancy grid over a scene set: windows, cell offsets, map and kernel settings, device pointers)."""
    _fields_ = [("scene_start", C.c_void_p), ("window", C.c_void_p), ("cell_start", C.c_void_p), ("maps", C.c_void_p),
                ("scene_map", C.c_void_p), ("map_from_world", C.c_void_p), ("cells", C.c_int64),
                ("offset", C.c_double * 2), ("step", C.c_double * 2), ("sigma", C.c_double), ("kernel_cut", C.c_double),
                ("num_scenes", C.c_int32), ("B_all", C.c_int32), ("n_sem", C.c_int32), ("num_maps", C.c_int32), ("map_h", C.c_int32),
                ("map_w", C.c_int32), ("drivable_layer", C.c_int32), ("no_map_fill", C.c_float)]


OCCUPANCY_MAX_WINDOW_CELLS = 1024      # include/cld.h CLD_OCCUPANCY_MAX_WINDOW_CELLS
OCCUPANCY_Q = float(1 << 40)           # the grid planes are Q40 fixed point

METRICS_AGENT_COLS = ("steps", "steps_valid", "off_road_sum", "off_road_disk_sum", "coll_any", "coll_front", "coll_rear", "coll_side",
                      "coll_disk", "failure_offroad", "failure_collision", "failure_any", "speed", "lon_acc", "lat_acc", "jerk")
METRICS_SCENE_COLS = 16      # include/cld.h CLD_METRICS_SCENE_COLS

GOAL_KINDS = {"global_target_pos": 1, "global_target_pos_at_time": 2}      # cld_goal.kind (0 = off)

_P = C.c_void_p
# name -> (restype, argtypes); every symbol include/cld.h declares
SIGNATURES = {
    "cld_default_config": (None, [C.POINTER(CldConfig)]),
    "cld_create": (C.c_int, [C.POINTER(CldConfig), C.POINTER(_P)]),
    "cld_destroy": (C.c_int, [_P]),
    "cld_last_error": (C.c_char_p, [_P]),
    "cld_load_weight": (C.c_int, [_P, C.c_char_p, _P, C.c_size_t]),
    "cld_finalize": (C.c_int, [_P, _P]),
    "cld_workspace_bytes": (C.c_size_t, [_P, C.c_int32]),
    "cld_get_schedule": (C.c_int, [_P, _P, _P, _P]),
    "cld_unet_forward": (C.c_int, [_P, _P, _P, C.c_int32, _P, C.c_int32, _P, C.c_size_t, _P]),
    "cld_unet_forward_t": (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, _P, C.c_size_t, _P]),
    "cld_denoise_loss": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_int32, _P, C.c_size_t, _P]),
    "cld_ddpm_step": (C.c_int, [_P, _P, _P, C.c_int32, _P, _P, _P, C.POINTER(C.c_float), C.c_int32, _P, C.c_size_t, _P]),
    "cld_sample": (C.c_int, [_P, _P, _P, _P, C.c_int32, _P, _P, _P, C.c_int32, C.c_uint64, _P, C.c_size_t, _P]),
    "cld_sample_cfg": (C.c_int, [_P, _P, _P, _P, _P, C.c_float, C.c_int32, _P, _P, _P, C.c_int32, C.c_uint64, _P, C.c_size_t, _P]),
    "cld_sample_guided": (C.c_int, [_P, _P, _P, _P, _P, C.c_float, C.POINTER(CldGuidance), C.c_int32, _P, _P, _P, C.c_int32,
                                    C.c_uint64, _P, C.c_size_t, _P]),
    "cld_sample_step": (C.c_int, [_P, _P, _P, _P, C.c_float, C.POINTER(CldGuidance), C.c_int32, _P, _P, _P, _P, _P, C.POINTER(C.c_float), C.c_int32, _P, C.c_size_t, _P]),
    "cld_guidance_step": (C.c_int, [_P, _P, _P, C.POINTER(CldGuidance), C.c_float, _P, _P, _P, _P, C.c_int32, _P, C.c_size_t, _P]),
    "cld_guidance_losses": (C.c_int, [_P, _P, C.POINTER(CldGuidance), _P, C.c_int32, _P]),
    "cld_log_prob": (C.c_int, [_P, _P, _P, _P, C.c_int32, _P, C.c_int32, _P, C.c_size_t, _P]),
    "cld_lstm_decode": (C.c_int, [_P, _P, _P, _P, C.c_int32, _P]),
    "cld_action_to_state": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P]),
    "cld_decode": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, _P]),
    "cld_traj2z": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_int32, _P]),
    "cld_vae_loss": (C.c_int, [_P, _P, _P, _P, _P, C.c_float, _P, C.c_int32, _P, C.c_size_t, _P]),
    "cld_state_to_state_and_action": (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, _P]),
    "cld_context_workspace_bytes": (C.c_size_t, [_P, C.c_int32]),
    "cld_context_encode": (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, _P, C.c_size_t, _P]),
    "cld_context_combine": (C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int32, _P]),
    "cld_compute_reward": (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_float, _P, _P, _P,
                                     C.c_int32, _P]),
    "cld_agent_collision": (C.c_int, [_P, _P, C.POINTER(CldCollision), _P, _P, _P, C.c_int32, _P]),
    "cld_map_collision_loss": (C.c_int, [_P, _P, C.POINTER(CldMapCollision), _P, _P, _P, C.c_int32, _P]),
    "cld_goal_loss": (C.c_int, [_P, _P, C.POINTER(CldGoal), _P, _P, _P, C.c_int32, _P]),
    "cld_set_goal_term": (C.c_int, [_P, C.POINTER(CldGoal)]),
    "cld_social_group_loss": (C.c_int, [_P, _P, C.POINTER(CldSocialGroup), _P, _P, _P, C.c_int32, _P]),
    "cld_set_social_term": (C.c_int, [_P, C.POINTER(CldSocialGroup)]),
    "cld_pair_loss": (C.c_int, [_P, _P, C.POINTER(CldPairTerm), _P, _P, _P, C.c_int32, _P]),
    "cld_set_pair_term": (C.c_int, [_P, C.POINTER(CldPairTerm)]),
    "cld_set_map_source": (C.c_int, [_P, C.POINTER(CldMapSource)]),
    "cld_world_step": (C.c_int, [_P, _P, _P, _P, C.c_int32, _P, _P, C.c_int32, _P]),
    "cld_rasterize": (C.c_int, [_P, C.POINTER(CldRaster), C.c_int32, C.c_int32, _P, _P, _P, _P]),
    "cld_scene_metrics_state_bytes": (C.c_size_t, [C.c_int32]),
    "cld_scene_metrics_step": (C.c_int, [_P, C.POINTER(CldSceneMetrics), _P, _P, _P, _P, C.c_int32, _P]),
    "cld_scene_metrics_read": (C.c_int, [_P, C.POINTER(CldSceneMetrics), _P, _P, _P, _P]),
    "cld_guide_metrics_state_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "cld_guide_metrics_step": (C.c_int, [_P, C.POINTER(CldGuideMetrics), _P, _P, _P, _P, C.c_int32, _P]),
    "cld_guide_metrics_read": (C.c_int, [_P, C.POINTER(CldGuideMetrics), _P, _P, _P, _P]),
    "cld_occupancy_splat": (C.c_int, [_P, C.POINTER(CldOccupancy), _P, _P, _P, _P]),
    "cld_occupancy_mark": (C.c_int, [_P, C.POINTER(CldOccupancy), _P, C.c_int32, _P, _P, _P]),
    "cld_occupancy_read": (C.c_int, [_P, C.POINTER(CldOccupancy), _P, _P, C.c_double, _P, _P, _P, _P, _P]),
    "cld_sort_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "cld_sort_f32": (C.c_int, [_P, _P, _P, C.c_int64, _P, C.c_size_t, _P]),
    "cld_wasserstein_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "cld_wasserstein_f32": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, _P, _P, C.c_size_t, _P]),
    "cld_realism_terms": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_float, _P, _P, _P, _P]),
    "cld_debug_sort_items_per_block": (C.c_int32, []),
    "cld_profile_enable": (C.c_int, [_P, C.c_int32]),
    "cld_profile_read": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "cld_profile_read_executed": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32)]),
    "cld_set_stride": (C.c_int, [_P, C.c_int32]),
    "cld_debug_lds_floor": (C.c_int, [_P, C.c_size_t]),
    "cld_debug_force_kernel": (C.c_int, [_P, C.c_int32, C.c_int32]),
    "cld_debug_conv5_form": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32]),
    "cld_debug_conv5_items": (C.c_int, [C.c_int32, C.c_int32, C.c_int64, C.c_int32]),
    "cld_debug_unet_span": (C.c_int, [_P, C.c_int32, _P, _P, _P, C.c_int32, _P, _P, C.c_int32, _P, C.c_size_t, _P]),
    "cld_debug_res_fold": (C.c_int, [_P, C.c_int32]),
    "cld_debug_pack_res_proj": (C.c_int64, [_P, C.c_int32, C.c_int32, _P, C.c_int64]),
    "cld_debug_context_layer": (C.c_int, [_P, C.c_int32, _P, _P, _P, C.c_int32, C.c_int32, _P]),
    "cld_debug_context_pass_size": (C.c_int, [C.c_int32]),
    "cld_debug_stamps": (C.c_int, [_P, _P, C.c_int32]),
    "cld_debug_guide_stamps": (C.c_int, [_P]),
    "cld_unet_param_count": (C.c_int, [_P]),
    "cld_unet_param_info": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                                      C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "cld_unet_param_floats": (C.c_size_t, [_P]),
    "cld_unet_tape_bytes": (C.c_size_t, [_P, C.c_int32]),
    "cld_unet_train_workspace_bytes": (C.c_size_t, [_P, C.c_int32]),
    "cld_unet_train_forward": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_size_t, C.c_int32, _P, C.c_size_t, _P]),
    "cld_unet_backward": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_size_t, _P, _P, _P, _P, C.c_int32, C.c_int32, _P, C.c_size_t, _P]),
    "cld_vae_param_count": (C.c_int, [_P]),
    "cld_vae_param_info": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                                     C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "cld_vae_param_floats": (C.c_size_t, [_P]),
    "cld_vae_tape_bytes": (C.c_size_t, [_P, C.c_int32, C.c_int32]),
    "cld_vae_train_workspace_bytes": (C.c_size_t, [_P, C.c_int32]),
    "cld_vae_encode_train": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, C.c_size_t, C.c_int32, _P]),
    "cld_vae_encode_backward": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_size_t, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, _P, C.c_size_t,
                                          _P]),
    "cld_vae_decode_train": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_size_t, C.c_int32, _P]),
    "cld_vae_decode_backward": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_size_t, _P, _P, _P, _P, C.c_int32, C.c_int32, _P, C.c_size_t, _P]),
    "cld_get_precision": (C.c_int, [_P]),
    "cld_version": (C.c_char_p, []),
}

# name -> (restype, argtypes); every symbol include/cld_lane.h declares (a table of its own: the one above is pinned to cld.h)
LANE_SIGNATURES = {
    "cld_lane_prepare": (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P]),
    "cld_lane_loss": (C.c_int, [_P, _P, C.POINTER(CldLaneTerm), _P, _P, _P, _P, C.c_int32, _P]),
    "cld_set_lane_term": (C.c_int, [_P, C.POINTER(CldLaneTerm)]),
}

class CldRecon(C.Structure):
    """include/cld_recon.h `cld_recon` (the flat U-Net buffer and the step settings of reconstruction guidance)."""
    _fields_ = [("params", C.c_void_p), ("lr", C.c_float), ("perturb_th", C.c_float), ("descend", C.c_int32)]


# name -> (restype, argtypes); every symbol include/cld_recon.h declares (a table of its own, as the lane table)
RECON_SIGNATURES = {
    "cld_recon_workspace_bytes": (C.c_size_t, [_P, C.c_int32, C.c_int32]),
    "cld_recon_step": (C.c_int, [_P, _P, _P, _P, C.c_float, C.POINTER(CldGuidance), C.POINTER(CldRecon), C.c_int32, _P, _P, _P, _P, _P, _P,
                                 C.POINTER(C.c_float), C.c_int32, C.c_uint64, C.c_uint64, _P, C.c_size_t, _P]),
    "cld_sample_recon": (C.c_int, [_P, _P, _P, _P, _P, C.c_float, C.POINTER(CldGuidance), C.POINTER(CldRecon), C.c_int32, _P, _P, _P,
                                   C.c_int32, C.c_uint64, _P, C.c_size_t, _P]),
    "cld_recon_get_posterior": (C.c_int, [_P, _P, _P]),
    "cld_debug_recon_grid_cap": (C.c_int32, [C.c_int32]),
}

class CldSolver(C.Structure):
    """include/cld_solver.h `cld_solver` (a few-step sampler: kind, K, a HOST pointer to K strictly decreasing timesteps, eta)."""
    _fields_ = [("kind", C.c_int32), ("n_steps", C.c_int32), ("timesteps", C.c_void_p), ("eta", C.c_float)]


SOLVER_KINDS = {"ddim": 0, "dpmpp_2m": 1}      # include/cld_solver.h CLD_SOLVER_*
SOLVER_TABLE_COLS = ("a", "b", "c0", "c1", "sqrt_recip_acp", "sqrt_recipm1_acp", "sigma", "sigma_g")      # CLD_SOLVER_TABLE_COLS

# name -> (restype, argtypes); every symbol include/cld_solver.h declares (a table of its own, as the lane table)
SOLVER_SIGNATURES = {
    "cld_solver_workspace_bytes": (C.c_size_t, [_P, C.c_int32, C.c_int32]),
    "cld_solver_tables": (C.c_int, [_P, C.POINTER(CldSolver), _P]),
    "cld_sample_solver": (C.c_int, [_P, C.POINTER(CldSolver), _P, _P, _P, _P, C.c_float, C.POINTER(CldGuidance), _P, C.c_int32, C.c_uint64,
                                    _P, C.c_size_t, _P]),
    "cld_solver_step": (C.c_int, [_P, C.POINTER(CldSolver), C.c_int32, _P, _P, _P, _P, _P, C.c_float, C.POINTER(CldGuidance), _P, _P, _P, _P, _P,
                                  C.c_int32, C.c_uint64, _P, C.c_size_t, _P]),
    "cld_debug_solver_grid_cap": (C.c_int32, [C.c_int32]),
    "cld_debug_solver_kernel": (C.c_int, [_P, C.POINTER(CldSolver), C.c_int32, _P, _P, _P, C.c_float, _P, _P, _P, _P, _P, C.c_int32, C.c_uint64, _P]),
}

# name -> (restype, argtypes); every symbol include/cld_eval.h declares (the open-loop sample metrics; a third table of its own)
EVAL_SIGNATURES = {
    "cld_sample_metrics_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "cld_sample_metrics": (C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_size_t, _P]),
    "cld_debug_sample_metrics_max_blocks": (C.c_int32, []),
}
# include/cld_eval.h CLD_SM_*: the columns of a per-agent row of cld_sample_metrics; the first eight under upstream's keys
# (DiffuserTrafficModel._compute_metrics), the last two this library's last-step pair distance
SAMPLE_METRIC_COLS = ("ego_avg_ADE", "ego_min_ADE", "ego_avg_FDE", "ego_min_FDE", "ego_avg_APD", "ego_max_APD", "ego_avg_FPD", "ego_max_FPD",
                      "ego_avg_last_step_PD", "ego_max_last_step_PD")
SAMPLE_METRIC_INDEX = ("best_ade", "best_fde", "last", "nonfinite")      # the columns of its int32 index rows
SAMPLE_METRICS_MAX_SAMPLES = 256       # include/cld_eval.h CLD_SM_MAX_SAMPLES
SAMPLE_METRICS_MAX_POINTS = 8192       # include/cld_eval.h CLD_SM_MAX_POINTS

_lib = None


def load():
    """Load libcld_hip.so (built by `__graft_entry__.build()` / `build.sh`); raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise CldError(f"{LIB_PATH} not found: build the HIP library first "
                       f"(python -c 'import __graft_entry__ as g; g.build()'). There is no CPU fallback.")
    # ONE HIP runtime per process: PyTorch-ROCm ships its own libamdhip64.so.7 (same SONAME as
    # /opt/rocm's).  Importing torch first makes libcld_hip.so bind to that already-loaded copy, so
    # torch's streams / device pointers and our launches live in the same runtime.  Loading this
    # library first would pull /opt/rocm's runtime in beside torch's and break device init.
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for table in (SIGNATURES, LANE_SIGNATURES, RECON_SIGNATURES, SOLVER_SIGNATURES, EVAL_SIGNATURES):
        for name, (res, args) in table.items():
            fn = getattr(lib, name)      # AttributeError if the library does not export it
            fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def check(handle, rc, what):
    if rc != 0:
        msg = load().cld_last_error(handle)
        raise CldError(f"{what} failed ({rc}): {msg.decode() if msg else '?'}")
