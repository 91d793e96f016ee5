"""ctypes mirror of include/po_hip.h (struct layouts and enums only; no behaviour)."""
PO_ABI_VERSION = 7  # include/po_hip.h
PO_NOT_AVAILABLE = -2  # po_info.status_refine / status_polish: asked for, no kernel for this shape
import ctypes as C

PO_KP, PO_KPC, PO_K = 0, 1, 2
PO_OK, PO_ERR_INVALID, PO_ERR_HIP, PO_ERR_UNSUPPORTED, PO_ERR_NOMEM = 0, -1, -2, -3, -4
PO_STATUS_SOLVED, PO_STATUS_MAX_ITER = 1, -2
PO_STATUS_PRIMAL_INFEASIBLE, PO_STATUS_DUAL_INFEASIBLE, PO_STATUS_UNSOLVED = -3, -4, -10
PO_STATUS_NON_FINITE = -8
FORM_BY_NAME = {"KP": PO_KP, "KPC": PO_KPC, "K": PO_K}  # OsqpSolver::create strings (solver.cpp:34-38)

_dp = C.POINTER(C.c_double)


class PoParams(C.Structure):
    _fields_ = [
        ("d", C.c_double * 4),
        ("w_curv", C.c_double), ("w_curv_rate", C.c_double), ("w_dev", C.c_double), ("w_slack", C.c_double),
        ("k_w_curv", C.c_double), ("k_w_curv_rate", C.c_double), ("k_w_dev", C.c_double),
        ("w_k_slack", C.c_double), ("w_kp_slack", C.c_double),
        ("margin", C.c_double), ("max_steer", C.c_double), ("wheel_base", C.c_double),
        ("constraint_end_heading", C.c_int), ("scaling", C.c_int),
        ("eps_abs", C.c_double), ("eps_rel", C.c_double), ("eps_prim_inf", C.c_double), ("eps_dual_inf", C.c_double),
        ("rho0", C.c_double), ("sigma", C.c_double), ("alpha", C.c_double), ("adapt_tol", C.c_double),
        ("max_iter", C.c_int), ("check_every", C.c_int), ("adapt_every", C.c_int), ("enable_collision_check", C.c_int),
        ("car_width", C.c_double), ("car_length", C.c_double), ("rear_axle_to_center", C.c_double), ("safety_margin", C.c_double),
        ("t2_w_dev", C.c_double), ("t2_w_curv", C.c_double), ("t2_w_curv_rate", C.c_double),
        ("cart_w_curv", C.c_double), ("cart_w_curv_rate", C.c_double), ("cart_w_dev", C.c_double),
        ("mu", C.c_double), ("max_curvature_rate", C.c_double), ("search_lateral_range", C.c_double),
        ("search_long_spacing", C.c_double), ("search_lat_spacing", C.c_double), ("enable_dynamic_segmentation", C.c_int), ("enable_raw_output", C.c_int), ("output_spacing", C.c_double), ("smoothing_method", C.c_int), ("optimization_method", C.c_int), ("enable_exact_position", C.c_int), ("polish", C.c_int),
        ("polish_delta", C.c_double), ("polish_refine_iter", C.c_int),
        ("refine", C.c_int), ("refine_eps", C.c_double), ("refine_rounds", C.c_int), ("refine_chain", C.c_int), ("refine_extra_rounds", C.c_int),
        ("refine_newton_rho", C.c_double), ("refine_newton_rho_eq", C.c_double), ("refine_newton_rho_max", C.c_double), ("refine_ls_tol", C.c_double), ("refine_ls_max", C.c_int), ("refine_newton_max", C.c_int), ("refine_newton_final", C.c_int), ("refine_newton_escalate", C.c_int), ("refine_newton_rho_eq_max", C.c_double),
    ]


class PoMap(C.Structure):
    _fields_ = [("distance", C.c_void_p), ("size_x", C.c_int), ("size_y", C.c_int), ("resolution", C.c_double),
                ("pos_x", C.c_double), ("pos_y", C.c_double)]


class PoOccupancy(C.Structure):
    _fields_ = [("cells", C.c_void_p), ("size_x", C.c_int), ("size_y", C.c_int), ("resolution", C.c_double),
                ("pos_x", C.c_double), ("pos_y", C.c_double)]


PO_OBS_DISC, PO_OBS_POLY, PO_OBS_MAX_VERTS = 0, 1, 8


class PoObstacle(C.Structure):  # 136 bytes; binding.OBSTACLE_DTYPE is the same layout as a numpy record
    _fields_ = [("kind", C.c_int), ("n_verts", C.c_int), ("v", C.c_double * 16)]


class PoObstacleLists(C.Structure):
    _fields_ = [("obs", C.c_void_p), ("first", C.c_void_p), ("n_obs", C.c_int), ("base", C.c_void_p), ("base_count", C.c_int),
                ("size_x", C.c_int), ("size_y", C.c_int), ("resolution", C.c_double), ("pos_x", C.c_double), ("pos_y", C.c_double)]


PO_RING_SOLID, PO_RING_FREE, PO_RING_MAX_VERTS, PO_WORLD_MAX_SIDE = 0, 1, 4096, 16384


class PoRings(C.Structure):
    _fields_ = [("verts", C.c_void_p), ("start", C.c_void_p), ("flags", C.c_void_p), ("n_rings", C.c_int), ("n_verts", C.c_int), ("n_shared", C.c_int),
                ("first", C.c_void_p)]


class PoScene(C.Structure):
    _fields_ = [("lists", PoObstacleLists), ("rings", PoRings), ("use_world", C.c_int)]


class PoInfo(C.Structure):
    _fields_ = [("status", C.c_int), ("iters", C.c_int), ("n_refactor", C.c_int), ("status_polish", C.c_int),
                ("r_prim", C.c_double), ("r_dual", C.c_double), ("rho", C.c_double), ("obj", C.c_double),
                ("status_refine", C.c_int), ("reserved", C.c_int)]


class PoBatchIn(C.Structure):
    _fields_ = [("formulation", C.c_int), ("B", C.c_int), ("N", C.c_int), ("keep", C.c_int),
                ("ref_x", C.c_void_p), ("ref_y", C.c_void_p), ("ref_z", C.c_void_p), ("ref_k", C.c_void_p),
                ("ref_s", C.c_void_p), ("bounds", C.c_void_p), ("x0", C.c_void_p), ("goal_z", C.c_void_p),
                ("max_k", C.c_void_p), ("max_kp", C.c_void_p), ("n_points", C.c_void_p), ("order", C.c_void_p)]


class PoBatchOut(C.Structure):
    _fields_ = [("states", C.c_void_p), ("info", C.c_void_p), ("x", C.c_void_p)]


INFO_DTYPE = [("status", "<i4"), ("iters", "<i4"), ("n_refactor", "<i4"), ("status_polish", "<i4"),
              ("r_prim", "<f8"), ("r_dual", "<f8"), ("rho", "<f8"), ("obj", "<f8"), ("status_refine", "<i4"), ("reserved", "<i4")]
INFO_BYTES = 56  # sizeof(po_info)


class PoBoundsIn(C.Structure):
    _fields_ = [("B", C.c_int), ("N", C.c_int), ("K", C.c_int),
                ("ref_x", C.c_void_p), ("ref_y", C.c_void_p), ("ref_z", C.c_void_p), ("ref_s", C.c_void_p), ("n_points", C.c_void_p),
                ("knot_s", C.c_void_p), ("knot_x", C.c_void_p), ("knot_y", C.c_void_p), ("n_knots", C.c_void_p)]


PO_SMOOTH_TENSION2, PO_SMOOTH_TENSION, PO_SMOOTH_POST = 0, 1, 2


class PoSmoothIn(C.Structure):
    _fields_ = [("kind", C.c_int), ("B", C.c_int), ("P", C.c_int), ("n_points", C.c_void_p),
                ("x", C.c_void_p), ("y", C.c_void_p), ("angle", C.c_void_p), ("k", C.c_void_p), ("s", C.c_void_p),
                ("lb", C.c_void_p), ("ub", C.c_void_p), ("l0", C.c_void_p)]


class PoSmoothOut(C.Structure):
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("s", C.c_void_p), ("info", C.c_void_p), ("raw", C.c_void_p)]


class PoSplineIn(C.Structure):
    _fields_ = [("B", C.c_int), ("K", C.c_int), ("knot_s", C.c_void_p), ("knot_x", C.c_void_p), ("knot_y", C.c_void_p),
                ("n_knots", C.c_void_p), ("length", C.c_void_p)]


class PoPlanIn(C.Structure):
    _fields_ = [("B", C.c_int), ("W", C.c_int), ("n_way", C.c_void_p), ("way_x", C.c_void_p), ("way_y", C.c_void_p), ("start", C.c_void_p),
                ("goal", C.c_void_p), ("max_length", C.c_double), ("N", C.c_int)]


class PoPlanOut(C.Structure):
    _fields_ = [("states", C.c_void_p), ("n_states", C.c_void_p), ("ok", C.c_void_p), ("stage", C.c_void_p), ("info", C.c_void_p)]


# ---- score and select (po_select_batch*) ----
PO_FEAT_LENGTH, PO_FEAT_CURV, PO_FEAT_CURV_RATE, PO_FEAT_KMAX, PO_FEAT_CLR_MIN, PO_FEAT_PROX, PO_FEAT_GOAL, PO_FEAT_DEV_PREV, PO_N_FEAT = 0, 1, 2, 3, 4, 5, 6, 7, 8


class PoSelectParams(C.Structure):
    _fields_ = [("w", C.c_double * PO_N_FEAT), ("d_safe", C.c_double), ("min_clearance", C.c_double), ("max_kmax", C.c_double), ("max_goal_dist", C.c_double)]


class PoSelectIn(C.Structure):
    _fields_ = [("B", C.c_int), ("N", C.c_int), ("states", C.c_void_p), ("n_states", C.c_void_p), ("ok", C.c_void_p), ("goal", C.c_void_p),
                ("goal_stride", C.c_int), ("G", C.c_int), ("group_start", C.c_void_p), ("Np", C.c_int), ("prev_states", C.c_void_p), ("prev_n", C.c_void_p)]


class PoSelectOut(C.Structure):
    _fields_ = [("feat", C.c_void_p), ("cost", C.c_void_p), ("best", C.c_void_p), ("best_cost", C.c_void_p), ("n_feasible", C.c_void_p),
                ("sel_states", C.c_void_p), ("sel_n", C.c_void_p)]


# ---- speed profile (po_speed_batch*) ----
class PoSpeedParams(C.Structure):
    _fields_ = [("v_max", C.c_double), ("a_lat_max", C.c_double), ("a_max", C.c_double), ("b_max", C.c_double), ("clear_v0", C.c_double),
                ("clear_gain", C.c_double), ("use_map", C.c_int)]


class PoSpeedIn(C.Structure):
    _fields_ = [("B", C.c_int), ("N", C.c_int), ("states", C.c_void_p), ("n_states", C.c_void_p), ("ok", C.c_void_p), ("v0", C.c_void_p),
                ("v_end", C.c_void_p), ("v_limit", C.c_void_p)]


class PoSpeedOut(C.Structure):
    _fields_ = [("v", C.c_void_p), ("a", C.c_void_p), ("t", C.c_void_p), ("total_time", C.c_void_p), ("status", C.c_void_p)]


# ---- moving obstacles (po_dynamic_batch*) ----
PO_AGENT_MAX_PTS, PO_AGENT_HOLD_BEFORE, PO_AGENT_HOLD_AFTER = 8, 1, 2


class PoAgent(C.Structure):  # 208 bytes; binding.AGENT_DTYPE is the same layout as a numpy record
    _fields_ = [("n_pts", C.c_int), ("flags", C.c_int), ("radius", C.c_double), ("t", C.c_double * PO_AGENT_MAX_PTS), ("x", C.c_double * PO_AGENT_MAX_PTS),
                ("y", C.c_double * PO_AGENT_MAX_PTS)]


class PoAgentLists(C.Structure):
    _fields_ = [("agents", C.c_void_p), ("first", C.c_void_p), ("n_agents", C.c_int), ("S", C.c_int)]


class PoDynamicParams(C.Structure):
    _fields_ = [("margin", C.c_double), ("stop_distance", C.c_double)]


class PoDynamicIn(C.Structure):
    _fields_ = [("B", C.c_int), ("N", C.c_int), ("states", C.c_void_p), ("n_states", C.c_void_p), ("ok", C.c_void_p), ("t", C.c_void_p), ("set_of", C.c_void_p),
                ("agents", C.POINTER(PoAgentLists)), ("v_limit_in", C.c_void_p)]


class PoDynamicOut(C.Structure):
    _fields_ = [("status", C.c_void_p), ("ok_out", C.c_void_p), ("gap_min", C.c_void_p), ("first_state", C.c_void_p), ("first_agent", C.c_void_p),
                ("stop_state", C.c_void_p), ("first_time", C.c_void_p), ("gap", C.c_void_p), ("v_limit", C.c_void_p)]


# ---- station-time speed planning (po_stplan_batch*) ----
PO_ST_MAX_LAYERS, PO_ST_MAX_STEP, PO_ST_MAX_STATIONS = 16, 31, 128


class PoStplanParams(C.Structure):
    _fields_ = [("dt", C.c_double), ("K", C.c_int), ("stride", C.c_int), ("U", C.c_int), ("margin", C.c_double), ("a_max", C.c_double), ("b_max", C.c_double),
                ("v_max", C.c_double), ("w_acc", C.c_double), ("w_slow", C.c_double)]


class PoStplanIn(C.Structure):
    _fields_ = [("B", C.c_int), ("N", C.c_int), ("states", C.c_void_p), ("n_states", C.c_void_p), ("ok", C.c_void_p), ("v0", C.c_void_p), ("v_cap", C.c_void_p),
                ("set_of", C.c_void_p), ("agents", C.POINTER(PoAgentLists)), ("v_limit_in", C.c_void_p)]


class PoStplanOut(C.Structure):
    _fields_ = [("status", C.c_void_p), ("ok_out", C.c_void_p), ("n_layers", C.c_void_p), ("cost", C.c_void_p), ("station", C.c_void_p), ("cells", C.c_void_p),
                ("v_limit", C.c_void_p)]


# ---- corridor nudge (po_nudge_batch*) ----
class PoNudgeParams(C.Structure):
    _fields_ = [("margin", C.c_double), ("t_before", C.c_double), ("t_after", C.c_double), ("min_width", C.c_double), ("skip_states", C.c_int)]


class PoNudgeIn(C.Structure):
    _fields_ = [("B", C.c_int), ("N", C.c_int), ("W", C.c_int), ("ref_x", C.c_void_p), ("ref_y", C.c_void_p), ("ref_z", C.c_void_p), ("n_points", C.c_void_p),
                ("ok", C.c_void_p), ("t", C.c_void_p), ("bounds", C.c_void_p), ("set_of", C.c_void_p), ("agents", C.POINTER(PoAgentLists)),
                ("side_prev", C.c_void_p)]


class PoNudgeOut(C.Structure):
    _fields_ = [("status", C.c_void_p), ("ok_out", C.c_void_p), ("bounds", C.c_void_p), ("side", C.c_void_p), ("first_blocked_state", C.c_void_p),
                ("first_blocked_agent", C.c_void_p), ("width_min", C.c_void_p)]


# ---- timed trajectory (po_trajectory_batch*) ----
PO_TRAJ_MAX_DISCS = 4


class PoTrajectoryParams(C.Structure):
    _fields_ = [("t0", C.c_double), ("dt", C.c_double), ("K", C.c_int), ("n_discs", C.c_int), ("disc_offset", C.c_double * PO_TRAJ_MAX_DISCS),
                ("disc_radius", C.c_double * PO_TRAJ_MAX_DISCS), ("agent_pts", C.c_int), ("agent_stride", C.c_int), ("agent_flags", C.c_int)]


class PoTrajectoryIn(C.Structure):
    _fields_ = [("B", C.c_int), ("N", C.c_int), ("states", C.c_void_p), ("n_states", C.c_void_p), ("ok", C.c_void_p), ("v", C.c_void_p), ("t", C.c_void_p)]


class PoTrajectoryOut(C.Structure):
    _fields_ = [("status", C.c_void_p), ("states", C.c_void_p), ("v", C.c_void_p), ("a", C.c_void_p), ("t", C.c_void_p), ("index", C.c_void_p),
                ("first_held", C.c_void_p), ("agents", C.c_void_p)]


# ---- agent sets (po_agentsets_batch*) ----
PO_SETS_SOURCES = 2


class PoAgentsetsParams(C.Structure):
    _fields_ = [("reach", C.c_double), ("t_before", C.c_double), ("t_after", C.c_double), ("win_lo", C.c_double), ("win_hi", C.c_double), ("owner_div", C.c_int)]


class PoAgentsetsIn(C.Structure):
    _fields_ = [("B", C.c_int), ("N", C.c_int), ("states", C.c_void_p), ("n_states", C.c_void_p), ("ok", C.c_void_p), ("t", C.c_void_p),
                ("src", C.POINTER(PoAgentLists) * PO_SETS_SOURCES), ("pool_of", C.c_void_p), ("owner", C.c_void_p)]


class PoAgentsetsOut(C.Structure):
    _fields_ = [("capacity", C.c_int), ("agents", C.c_void_p), ("first", C.c_void_p), ("count", C.c_void_p), ("status", C.c_void_p), ("set_of", C.c_void_p),
                ("src_index", C.c_void_p), ("total", C.c_void_p)]


# ---- stop, wait, go: station-time plans that resume, sampled in time (po_stgo_batch*) ----
class PoStgoParams(C.Structure):
    _fields_ = PoStplanParams._fields_ + [("t0", C.c_double), ("dts", C.c_double), ("Q", C.c_int)]


class PoStgoIn(C.Structure):
    _fields_ = [("B", C.c_int), ("N", C.c_int), ("states", C.c_void_p), ("n_states", C.c_void_p), ("ok", C.c_void_p), ("v0", C.c_void_p), ("v_cap", C.c_void_p),
                ("set_of", C.c_void_p), ("agents", C.POINTER(PoAgentLists))]


class PoStgoOut(C.Structure):
    _fields_ = [("status", C.c_void_p), ("ok_out", C.c_void_p), ("n_layers", C.c_void_p), ("cost", C.c_void_p), ("station", C.c_void_p), ("cells", C.c_void_p),
                ("n_resumes", C.c_void_p), ("states", C.c_void_p), ("v", C.c_void_p), ("a", C.c_void_p), ("t", C.c_void_p), ("index", C.c_void_p),
                ("first_held", C.c_void_p), ("end", C.c_void_p)]


# ---- speed QP: a jerk-limited s(t) inside a station-time plan's free tunnel (po_speedqp_batch*) ----
PO_SQP_MAX_SAMPLES = 256


class PoSpeedqpParams(C.Structure):
    _fields_ = [("dt", C.c_double), ("K", C.c_int), ("stride", C.c_int), ("v_max", C.c_double), ("dts", C.c_double), ("Q", C.c_int),
                ("a_max", C.c_double), ("b_max", C.c_double), ("j_max", C.c_double), ("w_s", C.c_double), ("w_a", C.c_double), ("w_j", C.c_double),
                ("rho", C.c_double), ("sigma", C.c_double), ("alpha", C.c_double), ("eps_abs", C.c_double), ("eps_rel", C.c_double),
                ("max_iter", C.c_int), ("check_every", C.c_int), ("adaptive_rho", C.c_int)]


class PoSpeedqpIn(C.Structure):
    _fields_ = [("B", C.c_int), ("N", C.c_int), ("states", C.c_void_p), ("n_states", C.c_void_p), ("ok", C.c_void_p), ("v0", C.c_void_p), ("v_cap", C.c_void_p),
                ("station", C.c_void_p), ("n_layers", C.c_void_p), ("cells", C.c_void_p), ("ref_states", C.c_void_p)]


class PoSpeedqpOut(C.Structure):
    _fields_ = [("status", C.c_void_p), ("iters", C.c_void_p), ("n_fact", C.c_void_p), ("r_prim", C.c_void_p), ("r_dual", C.c_void_p), ("n_q", C.c_void_p),
                ("states", C.c_void_p), ("v", C.c_void_p), ("a", C.c_void_p), ("jerk", C.c_void_p), ("t", C.c_void_p), ("lo", C.c_void_p), ("hi", C.c_void_p),
                ("index", C.c_void_p)]
