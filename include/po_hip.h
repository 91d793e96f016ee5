/*
 * po_hip.h — C ABI of libpo_hip.so, the MI355X (gfx950) batched QP path-optimisation engine.
 *
 * This is the drop-in boundary for the reference's OSQP wrapper.  The reference has no FFI layer:
 * its lower edge is the OsqpEigen::Solver member used in
 *     /root/reference/src/solver/solver.cpp:46-77            (OsqpSolver::solve)
 * and its upper edge is
 *     /root/reference/include/path_optimizer/solver/solver.hpp:31-36
 *         OsqpSolver::create(type, ReferencePath&, VehicleState&, horizon) / solve(std::vector<State>*)
 * called only from /root/reference/src/path_optimizer/path_optimizer.cpp:182-183.
 * Everything between those two edges (Hessian/constraint/bound assembly, the ADMM iteration, the
 * Frenet->Cartesian output map) runs behind the entry points below.  Plain pointers and sizes only.
 *
 * All floating point data is IEEE double ("f64"), as in the reference.
 */
#ifndef PO_HIP_H_
#define PO_HIP_H_

#ifdef __cplusplus
extern "C" {
#endif

/* ---- formulations: the three subclasses OsqpSolver::create() can return (solver.cpp:30-44) ---- */
enum {
    PO_KP  = 0, /* "KP"  SolverKpAsInput            src/solver/solver_kp_as_input.cpp             */
    PO_KPC = 1, /* "KPC" SolverKpAsInputConstrained src/solver/solver_kp_as_input_constrained.cpp */
    PO_K   = 2  /* "K"   SolverKAsInput             src/solver/solver_k_as_input.cpp              */
};

/* ---- API return codes (never abort; the reference's CHECK_* aborts become codes) ---- */
enum {
    PO_OK              = 0,
    PO_ERR_INVALID     = -1, /* bad argument (null pointer, N < 2, unknown formulation, ...) */
    PO_ERR_HIP         = -2, /* a HIP runtime call failed; po_last_hip_error() has the text  */
    PO_ERR_UNSUPPORTED = -3, /* problem does not fit the device tile (N too large)           */
    PO_ERR_NOMEM       = -4
};

/* ---- per-path solver status; values follow OSQP's so that "solved" == 1 maps to the
 *      reference's `solver_.solve()` returning true (OsqpEigen returns true only for OSQP_SOLVED) ---- */
enum {
    PO_STATUS_SOLVED            = 1,
    PO_STATUS_MAX_ITER          = -2,
    PO_STATUS_PRIMAL_INFEASIBLE = -3,
    PO_STATUS_DUAL_INFEASIBLE   = -4,
    PO_STATUS_NON_FINITE        = -8, /* not an OSQP value: a NaN / Inf appeared in the iterate (non-finite inputs); never reported as solved */
    PO_STATUS_UNSOLVED          = -10
};

/* Parameter block.  Replaces the gflags globals the reference reads during assembly
 * (src/config/planning_flags.cpp:8-14,18-43,102-119) plus the OSQP settings
 * (reference touches only verbosity/warm_start, src/solver/solver.cpp:48-49; the rest are
 * OSQP defaults, except eps which this project's metric fixes at 1e-4). Immutable after po_create. */
typedef struct po_params {
    double d[4];            /* FLAGS_d1..d4: rear-axle -> covering-circle centre offsets.  NOT derived by the library: a caller that changes car_length or
                               rear_axle_to_center sets d[j] = ((2 j - 3) / 8) * car_length + rear_axle_to_center itself (the reference's updateConfig,
                               planning_flags.cpp:10-13); the path QP and po_bounds_batch* read d as given.  The covering-circle radius of po_bounds_batch* IS
                               derived, from car_length, car_width and safety_margin (FLAGS_circle_radius, planning_flags.cpp:9), at every call.
                               The vehicle fields (d, car_width, car_length, rear_axle_to_center, safety_margin) are not validated anywhere: a non-positive
                               or NaN value is used as it stands and the results of the stages that read it are unspecified (tests/test_settings.py).     */
    double w_curv;          /* FLAGS_KP_curvature_weight       (10)                                */
    double w_curv_rate;     /* FLAGS_KP_curvature_rate_weight  (200)                               */
    double w_dev;           /* FLAGS_KP_deviation_weight       (0)                                 */
    double w_slack;         /* FLAGS_KP_slack_weight           (3)  (also used by K, k_as_input.cpp:54) */
    double k_w_curv;        /* FLAGS_K_curvature_weight        (50)                                */
    double k_w_curv_rate;   /* FLAGS_K_curvature_rate_weight   (200)                               */
    double k_w_dev;         /* FLAGS_K_deviation_weight        (0)                                 */
    double w_k_slack;       /* KPC literal 500    (solver_kp_as_input_constrained.cpp:52)          */
    double w_kp_slack;      /* KPC literal 25000  (solver_kp_as_input_constrained.cpp:53)          */
    double margin;          /* FLAGS_expected_safety_margin    (1.3)                               */
    double max_steer;       /* FLAGS_max_steering_angle        (30 deg)                            */
    double wheel_base;      /* FLAGS_wheel_base                (2.85)                              */
    int    constraint_end_heading; /* FLAGS_constraint_end_heading (true)                          */
    int    scaling;         /* equilibration passes: 10 = OSQP default (the reference never changes it);
                               the engine runs the class-level form of Ruiz; 0 = off  */
    /* ADMM (OSQP names) */
    double eps_abs, eps_rel;            /* 1e-4, 1e-4 (project metric; OSQP default is 1e-3)       */
    double eps_prim_inf, eps_dual_inf;  /* 1e-4, 1e-4                                              */
    double rho0, sigma, alpha;          /* 0.1, 1e-6, 1.6                                          */
    double adapt_tol;                   /* adaptive_rho_tolerance 5                                */
    int    max_iter;                    /* 4000                                                    */
    int    check_every;                 /* check_termination 25                                    */
    int    adapt_every;                 /* adaptive-rho interval in iterations (100 = OSQP's
                                           non-profiling default 4*check_termination); 0 = off     */
    int    enable_collision_check;      /* FLAGS_enable_collision_check (true), post-solve step only */
    /* vehicle footprint, read by the post-solve collision check (planning_flags.cpp:18-29) */
    double car_width;           /* FLAGS_car_width           (2.0)  */
    double car_length;          /* FLAGS_car_length          (4.9)  */
    double rear_axle_to_center; /* FLAGS_rear_axle_to_center (1.45) */
    double safety_margin;       /* FLAGS_safety_margin       (0.0): circle_radius = sqrt((L/8)^2+(W/2)^2) + safety_margin */
    /* reference-smoothing QPs, planning_flags.cpp:76-86 */
    double t2_w_dev;            /* FLAGS_tension_2_deviation_weight       (0.005) */
    double t2_w_curv;           /* FLAGS_tension_2_curvature_weight       (1)     */
    double t2_w_curv_rate;      /* FLAGS_tension_2_curvature_rate_weight  (10)    */
    double cart_w_curv;         /* FLAGS_cartesian_curvature_weight       (1)     */
    double cart_w_curv_rate;    /* FLAGS_cartesian_curvature_rate_weight  (50)    */
    double cart_w_dev;          /* FLAGS_cartesian_deviation_weight       (0)     */
    /* re-sampling, limits and the DP lattice search, planning_flags.cpp:41-43,57-63,137 */
    double mu;                  /* FLAGS_mu                          (0.4)  */
    double max_curvature_rate;  /* FLAGS_max_curvature_rate          (0.1)  */
    double search_lateral_range;   /* FLAGS_search_lateral_range        (10.0) */
    double search_long_spacing;    /* FLAGS_search_longitudial_spacing  (1.5)  */
    double search_lat_spacing;     /* FLAGS_search_lateral_spacing      (0.6)  */
    int    enable_dynamic_segmentation; /* FLAGS_enable_dynamic_segmentation (true) */
    int    enable_raw_output;           /* FLAGS_enable_raw_output (true): output the QP states directly; false: densify through a spline */
    double output_spacing;              /* FLAGS_output_spacing (0.3) */
    /* po_plan_batch only: which smoother QP and which path formulation the chain uses */
    int    smoothing_method;            /* FLAGS_smoothing_method: PO_SMOOTH_TENSION2 (default "TENSION2") or PO_SMOOTH_TENSION ("TENSION") */
    int    optimization_method;         /* FLAGS_optimization_method: PO_KP (default "KP"), PO_K ("K") or PO_KPC */
    int    enable_exact_position;       /* FLAGS_enable_exact_position (false): goal-trim search step 0.1 m instead of 0.5 m (path_optimizer.cpp:151) */
    int    polish;                      /* OSQP `polish` (0 = off: OSQP's default, which the reference never changes).  1: after a path is solved, the reduced
                                           KKT system on the active set is solved with the regularisation `polish_delta` and `polish_refine_iter` steps of
                                           iterative refinement (OSQP polish.c); the result replaces the ADMM solution when OSQP's acceptance rule holds.  Shapes
                                           without a polish kernel (KP keep 6 .. 16, and the single-level mapping): po_info.status_polish = PO_NOT_AVAILABLE */
    double polish_delta;                /* OSQP `delta` (1e-6) */
    int    polish_refine_iter;          /* OSQP `polish_refine_iter` (3) */
    /* Refinement (extension, off by default; runs after a path is solved and before the polish).  refine = 2: semismooth Newton on the augmented Lagrangian
     *     phi_y(x) = 1/2 x'Px + sum_i rho_i / 2 dist^2(a_i x + y_i / rho_i, [l_i, u_i])
     * (rho_i = refine_newton_rho on inequality rows, refine_newton_rho_eq on equality rows, scaled problem) with a line search on the piecewise-quadratic merit (safeguarded
     * Newton on its piecewise-linear derivative, run to refine_ls_tol), and a multiplier update  y <- rho (w - clip(w))  whenever the inner problem is solved to the dual
     * tolerance.  Each Newton step is ONE factorisation of the same block-tridiagonal matrix the ADMM iteration uses, with the rows outside their bounds at rho_i and the
     * others at OSQP's RHO_MIN, one solve, and a few row passes for the line search; the method is monotone in phi and terminates finitely.  It runs from the point the
     * OSQP-faithful ADMM iteration stops at (refine_rounds: how early) until OSQP's termination test holds at refine_eps (po_info.status_refine = 1: certified).
     * po_info.iters counts a Newton step as one iteration.  On BASELINE config 3 every path ends within 1e-4 m of the exact optimum (39 % at eps 1e-4 without).
     * Values: 0 off (the library default: OSQP-faithful), 2 on.  (ABI 5 removed refine = 1 — the activity-weighted ADMM continuation of rounds 2 - 3 —, its knobs
     * refine_every / refine_max_iter / refine_max_refactor / refine_rho / refine_adapt, the chained-rounds scheduling refine_chain 0 / 1 with refine_speculate, probe_iters
     * and polish_passes: the Newton phase in its own launches is faster on every shape, profiles/README.md; po_create returns PO_ERR_INVALID for refine = 1.) */
    int    refine;
    double refine_eps;                  /* 1e-7: eps_abs = eps_rel of the termination test of this phase (what po_info.status_refine = 1 certifies).  Measured on all 4096
                                           paths of BASELINE config 3 against their exact optima: certified at 1e-7 -> max e_y RMS error 1e-5 m; at 1e-6 seven certified
                                           paths were 1e-4 .. 4e-4 m away (these QPs are flat: e_y is the double integral of the curvature) */
    int    refine_rounds;               /* 1.  R > 1: the solve first stops at 10^(R-1) x (eps_abs, eps_rel) and is refined from there; a path the refinement does not
                                           certify at refine_eps goes back to the type-based iteration at a 10 x tighter eps and is refined again, down to eps itself.
                                           Every path returned satisfies OSQP's test at eps_abs / eps_rel or at refine_eps.  The headline setting uses 5: the ADMM
                                           iteration is then only a 25-iteration warm start (its first termination check passes at 1e4 x eps) */
    int    refine_chain;                /* 2 (default) or 3; scheduling only, results bit-identical.  The solve is three launches on one stream: the plain solve kernels as the
                                           warm start, the Newton refinement of round 0 as a launch of its own, and a fallback launch that takes the paths it did not
                                           certify (rare) through their later rounds.  2: the fallback launch is issued only when a path needs it — the engine reads a
                                           4-byte count back, so the device-pointer entry returns when the Newton launch has FINISHED (it blocks; the launch it saves
                                           costs 0.5 ms; a stream that is being captured is detected and treated as 3 — warm the handle up with one eager call of the
                                           same shape first: a handle does not allocate during capture); 3: always issued, fully asynchronous. */
    int    refine_extra_rounds;         /* 0.  E > 0: a path that the last regular round does not certify at refine_eps continues BELOW eps — type-based iteration at
                                           eps / 10, refinement again, eps / 100, ... — for up to E more rounds.  A path returned after them is certified, or satisfies
                                           OSQP's test at eps / 10^E — or ran out of max_iter in one of these rounds: then the point it ends on is tested against OSQP's
                                           criteria at the caller's eps once more — passes: that point, PO_STATUS_SOLVED with status_refine -1; fails (ADMM residuals are
                                           not monotone): the point that round STARTED from (it met eps in the round before), PO_STATUS_SOLVED with status_refine -1.  A
                                           round below eps never turns a solved path into MAX_ITER. */
    double refine_newton_rho;           /* 100 (scaled problem): penalty of the inequality rows at the start of an attempt; it grows 10 x whenever a multiplier update does not cut the
                                           primal residual by 4.  Measured on the whole BASELINE batches (oracle): 100 needs the fewest steps AND has the shortest tail (config 3:
                                           mean 14.8 / max 40 Newton steps; 1e3: 16.1 / 52; 1e4: 18.4 / 240; 30: 16.3 / 40 but 4 of 512 narrow-corridor paths uncertified) */
    double refine_newton_rho_eq;        /* 1e4: penalty of the equality rows at the start of an attempt (NOT 1e3 x the inequality one as in OSQP's step vector: the merit's
                                           gradient carries rho_eq x (a.x - b), a difference of O(1) numbers, whose rounding at rho_eq >= 1e6 sits near the dual tolerance);
                                           raised only for a path whose multiplier updates stall, see refine_newton_rho_eq_max */
    double refine_newton_rho_max;       /* 1e5: a multiplier update that does not cut the primal residual by 4 raises the penalty 10 x, up to this (the slow
                                           case: active rows that are nearly dependent through the heavily weighted curvature-rate variables).  <= 0: the default;
                                           at most OSQP's RHO_MAX = 1e6, which also bounds what refine_newton_escalate raises it to */
    double refine_ls_tol;               /* 0.6: the line search stops at |psi'(t)| <= tol |psi'(0)| (the search is a safeguarded Newton iteration on the piecewise-linear psi', so
                                           what it accepts is close to the root anyway).  Measured on the whole BASELINE batches, every path certified at every setting: 1e-4 -> 0.3
                                           3 - 7 % fewer Newton steps and 14 % fewer evaluations per step (round 4); 0.3 -> 0.6 another 1 % fewer steps, the first trial step
                                           accepted more often (config 3 5.19 -> 4.98 ms, config 5 21.3 -> 19.6 ms) and the SAME largest distance from the exact optimum on every
                                           golden batch (2.1e-5 m); 0.9 is 3 % faster again but lands 3 paths of config 5 (KPC, flat directions) at 5 - 6.5e-5 m, half the margin
                                           to the 1e-4 m bar (round 5).  The final correction steps always search to 1e-4. */
    int    refine_ls_max;               /* 30: evaluations of psi' per line search at most */
    int    refine_newton_max;           /* 300: Newton steps per attempt (every round).  BASELINE config 3: mean 16, max 60; config 5 (KPC): mean 28, max ~210 */
    int    refine_newton_final;         /* 3: once the point is certified at refine_eps, Newton steps go on (tight line search, no multiplier update) until the dual residual — the
                                           gradient of the merit — sits 1e3 x below its tolerance, at most this many (none when it already does at certification).  Newton converges
                                           quadratically once the active set is right, so this is normally ONE step to the rounding floor: the accuracy a tighter refine_eps would
                                           buy, without asking the termination test for tolerances below what fp64 delivers on the KPC rows weighted 1e5 (measured: refine_eps 3e-9
                                           leaves 93 of 4096 KPC paths stalling at r_dual 5e-9 until the step budget is spent).  Exactly one step is not enough: a step that changes
                                           the active set can land with a LARGER dual residual than the certified point's (2 of 4096 KPC paths ended 1.06e-4 m from their optimum
                                           that way; the offset e_y carries no cost of its own, so a gradient of 1e-7 is 1e-4 m there).  0: stop at the certified point. */
    int    refine_newton_escalate;      /* 12: from this many multiplier updates of an attempt on, refine_newton_rho_max and refine_newton_rho_eq_max stand 10 x higher, from twice as
                                           many on 100 x.  For DEGENERATE optima (linearly dependent active rows — corridors narrower than the soft margin produce them): the
                                           multipliers are not unique, the method of multipliers converges sublinearly at any fixed penalty (measured: the primal residual falls
                                           0.4 % per update at 1.2 x its tolerance), and only a larger penalty shortens it.  On the narrow-corridor batch of `host_test bench`: 2 of
                                           4096 paths uncertified and 15 - 18 through the fall-back rounds (12 - 27 ms) without it, none with it; no BASELINE path gets that far.  0: off. */
    double refine_newton_rho_eq_max;    /* 1e6: once the inequality penalty sits at refine_newton_rho_max and a multiplier update still does not cut the primal residual by 4,
                                           the EQUALITY rows' penalty grows 10 x instead, up to this.  The case: the primal residual left on the dynamics rows, whose multipliers
                                           converge at H / (H + rho_eq) per update when the active inequality rows beside them carry 10 x their penalty (wide corridors with a
                                           large initial offset: 24 of 4096 paths of `host_test bench` ran out of updates uncertified without it; config 5: hardest path 222 -> 129).
                                           0: the equality penalty never grows; < 0: the default; at most 1e8, which also bounds what refine_newton_escalate raises it to */
} po_params;

#define PO_NOT_AVAILABLE (-2) /* po_info.status_refine / status_polish: asked for, but the batch's shape has no kernel for it (see the fields) */
typedef struct po_info {
    int    status;      /* PO_STATUS_*                                  */
    int    iters;       /* ADMM iterations run (with po_params.refine: the solve's and the refinement's together) */
    int    n_refactor;  /* numeric refactorisations after the first (the refinement's included) */
    int    status_polish; /* OSQP info.status_polish: 0 not attempted (polish off, or the path was not solved), 1 polished solution adopted, -1 polish unsuccessful
                             (ADMM solution kept); PO_NOT_AVAILABLE (-2): po_params.polish was set but the SHAPE of this batch has no polish kernel — the role-split
                             mapping (KP, keep_control_steps_ 6 .. 16) and the single-level mapping (see status_refine) — the solve itself is unaffected */
    double r_prim;      /* ||Ax - z||_inf   at exit (unscaled)          */
    double r_dual;      /* ||Px + q + A'y||_inf at exit                 */
    double rho;         /* final rho                                    */
    double obj;         /* 0.5 x'Px at exit                             */
    int    status_refine; /* po_params.refine: 0 the refinement did not run on this path (refine off, or the path was not solved); 1 CERTIFIED: OSQP's
                             termination test holds ON THE RETURNED POINT at refine_eps (default 1e-7; re-evaluated after every step, the final correction steps included:
                             ABI 5), i.e. the point is the QP's optimum to that tolerance; -1 the
                             refinement ran out of its budget before that: the returned point satisfies OSQP's test at eps_abs / eps_rel only (it is the refined
                             point when its residuals are no worse than the solved point's, else the solved point) — a caller that needs the <= 1e-4 m accuracy
                             clause per path treats -1 as "not certified";
                             PO_NOT_AVAILABLE (-2, ABI 6): po_params.refine = 2 was set but the SHAPE of this batch has no Newton kernel, so the call ran the plain solve at
                             eps_abs / eps_rel on every path (status is what that solve reports).  The shapes WITH one — every case the reference's own pipeline produces
                             (keep_control_steps_ 1 .. 8 from 0.15 .. 1.0 m spacing, path_optimizer.cpp:171-172; the reference itself accepts any horizon_,
                             solver_kp_as_input.cpp:13-24): KP keep 1 .. 4 up to N = 512, keep 5 up to N = 320, keep 6 .. 8 up to N = 64 keep, keep 9 .. 16 up to
                             N = 32 keep; KPC (keep 4) and K up to N = 512; in every case only while the two-level tables fit 160 KB of LDS.  Without one (the single-level
                             chain): keep > 16, and longer paths than those limits. */
    int    reserved;
} po_info;

/* One homogeneous batch: B independent paths, each with N points and the same `keep`
 * (keep_control_steps_, solver_kp_as_input.cpp:17; ignored for PO_K; must be 4 for PO_KPC,
 * solver_kp_as_input_constrained.cpp:17).  All arrays are row-major, path-major.
 * Replaces the reads of ReferencePath::{getReferenceStates,getBounds,getMaxKList,getMaxKpList}
 * (include/path_optimizer/data_struct/reference_path.hpp:34-37) and
 * VehicleState::{getInitError,getStartState,getEndState}
 * (include/path_optimizer/data_struct/vehicle_state_frenet.hpp:18-23). */
typedef struct po_batch_in {
    int formulation, B, N, keep;
    const double *ref_x, *ref_y, *ref_z, *ref_k, *ref_s; /* [B][N]  State.{x,y,z,k,s}              */
    const double *bounds;   /* [B][N][4][2]: circles c0..c3 x {lb (right, <=0), ub (left, >=0)}    */
    const double *x0;       /* [B][3]: init_offset, init_heading_error, start_state.k               */
    const double *goal_z;   /* [B]: end_state.z                                                     */
    const double *max_k;    /* [B][N] KPC only (else NULL)                                          */
    const double *max_kp;   /* [B][N] KPC only; indexed by CONTROL id like the reference (:179-183) */
    const int    *n_points; /* optional [B]: points of each path, 2 <= n_points[b] <= N (ragged batch); NULL = all N.
                               Every array keeps its stride N; outputs beyond n_points[b] are zero.              */
    const int    *order;    /* optional [B]: a PERMUTATION of 0..B-1; workgroup i solves path order[i] (workgroups start in index order).  A scheduling
                               hint only — results do not depend on it: a launch ends with its longest path, so a caller that re-solves similar
                               problems every planning cycle passes the paths sorted by the previous cycle's po_info.iters, longest first.
                               NULL = the engine's own XCD-aware mixing of the path order. */
} po_batch_in;

typedef struct po_batch_out {
    double  *states; /* [B][N][5]: x, y, heading, k, s  (State.v = State.a = 0 in the reference)   */
    po_info *info;   /* [B]                                                                         */
    double  *x;      /* optional [B][n]: raw QP solution in the REFERENCE variable order, or NULL   */
} po_batch_out;

/* Obstacle-distance map: what the reference reads through PathOptimizationNS::Map::getObstacleDistance / isInside
 * (src/tools/Map.cpp:16-26), i.e. layer "distance" of a grid_map::GridMap sampled with
 * atPosition(INTER_LINEAR).  grid_map is a third-party dependency that is NOT in /root/reference (ROS package
 * grid_map_core, un-pinned): its geometry conventions are restated in csrc/po_map.hpp / oracle/po_oracle.c:
 * `distance` is the layer's Eigen::MatrixXf, column-major, size_x rows (along x) by size_y columns (along y);
 * cell (0,0) is the corner of LARGEST x and y; cell (i,j) is centred at
 *   pos + 0.5*len - (idx + 0.5)*resolution,  len = size*resolution;  the circular-buffer start index is (0,0). */
typedef struct po_map {
    const float *distance;  /* [size_y][size_x] in memory (column-major), metres to the nearest obstacle */
    int    size_x, size_y;
    double resolution;      /* metres per cell */
    double pos_x, pos_y;    /* position of the map centre in the world frame */
} po_map;

typedef struct po_handle_s *po_handle;

/* Fill `p` with the reference defaults (planning_flags.cpp) and the project's ADMM settings. */
void po_default_params(po_params *p);

/* QP dimensions exactly as the reference constructors compute them
 * (solver_kp_as_input.cpp:13-24, solver_kp_as_input_constrained.cpp:13-24, solver_k_as_input.cpp:14-20). */
int po_problem_dims(int formulation, int N, int keep, int *n, int *m, int *C);

/* keep_control_steps_ from the first <=9 arc-length gaps, with the reference's truncation
 * (solver.cpp:22-27 + solver_kp_as_input.cpp:17). Returns keep (>=1) or PO_ERR_INVALID. */
int po_keep_control_steps(int formulation, const double *ref_s, int N);

/* Number of HIP devices visible to the process (0 when there is none, or no driver): one handle per device is how a batch is spread over the GPUs of a
 * node (host/include/path_optimizer_amd/solver.hpp: OsqpSolver::solveBatch over several PoEngine). */
int po_device_count(void);
/* One handle = one HIP device + one stream.  Distinct handles (same device or not) may be used concurrently from different host threads.
 * ONE handle may be called from several host threads too, on any of its entries: each call is atomic — a host-pointer entry (and po_plan_batch*) holds the handle's
 * call lock from before it stages its inputs until its results have been read back, so no other call sees or reuses its staging blocks in between; a device-pointer
 * entry takes the handle's inner lock while it enqueues, owns no staging, and its scratch is ordered by the stream.  The library orders the calls; every call returns
 * what it would return in SOME serial order of the calls, i.e. what the same call returns on a handle nobody else uses (results do not depend on what a handle ran
 * before: tests/test_handle_contract.py).  Two calls on one handle never overlap on the device — use two handles for that.
 * Stream capture: after one eager warm-up call of the same shape on the handle (a handle does not allocate during capture; po_select_batch_device grows its scratch in
 * that call), po_solve_batch_device, po_speed_batch_device, po_trajectory_batch_device, po_dynamic_batch_device, po_stplan_batch_device, po_nudge_batch_device and
 * po_select_batch_device only enqueue and may be captured into a graph on the handle's stream, alone or as a chain; po_plan_batch_device synchronises the stream between
 * its groups and may NOT be captured.
 * NOT guaranteed: a thread that calls po_set_stream / po_set_map / po_set_map_occupancy* / po_set_map_stack* (po_set_map_stack_obstacles* and po_set_map_stack_scene* included) / po_set_world_occupancy* /
 * po_set_map_assignment* / po_debug_set while other threads solve on the same handle gets what it asked for — calls that
 * start afterwards use the new stream / map / switch, and the caller orders what is already enqueued on the old stream.  po_last_kernel_ms / po_last_phase_ms
 * describe the handle's last solve, whichever thread made it.  po_destroy must not race with any call. */
int po_create(int device, const po_params *params, po_handle *out);
int po_destroy(po_handle h);
/* Use an existing hipStream_t (e.g. torch's current stream); NULL = the handle's own stream. */
int po_set_stream(po_handle h, void *hip_stream);
/* Developer switches for A/B measurements and tests (the library reads NO environment variable; results never depend on these).  Keys: "identity_order" (workgroup i
 * solves path i instead of the XCD-aware mixing), "debug_cycles" (per-phase shader clocks of path 0 on stderr; makes the solve entry synchronous), "host_threads",
 * "smooth_seq", "smooth_waves", "smooth_nopad", "smooth_debug" (smoothing-QP engine variants), "dp_one_wave" (DP lattice search on one wave per instance whatever
 * the batch size), "newton_slice" (refine = 2: Newton steps of the FIRST of the two Newton launches, default 8 — every path runs that many, what is unfinished is parked
 * and the second launch takes the parked paths in order of expected remaining work, longest first; 0: one launch; left alone the engine slices batches of
 * at least two rounds of the device's wave slots (2 x 4 x CUs = 2048 paths) on shapes that run one wave per path, a value set here applies to every batch.  Scheduling only: the same operations in the same
 * order — statuses and certificates do not depend on it, the solutions agree to round-off (the kernels of the two launches are compiled separately; identical bit for bit on the
 * BASELINE KP / K shapes, <= 1e-10 elsewhere); BASELINE config 3: 4.76 -> 4.06 ms), "fixed_length" (default 1; 0: the generic kernels also for the path lengths the library was built with kernels
 * of their own for — the Makefile's PO_FIXED_N, KP with keep 4, non-ragged batches of exactly such a length; same operations in the same order, separately compiled),
 * "fixed_classes" (default 1; 0: the Newton launches of those lengths without the constant-class kernels, which take every path whose stage-local rows are all
 * inequalities and leave the others to the kernels without the constants; bit for bit the same results).
 * Unknown key: PO_ERR_INVALID. */
int po_debug_set(po_handle h, const char *key, int value);
/* Developer read-back (synchronises the stream): "fallback_paths" = how many paths the Newton launch of the last solve with refine = 2 did not certify and handed to
 * the fallback launch; "newton_parked" = how many went on into the second of the sliced Newton launches (-1: the last solve was not sliced); "map_ptr" = the device
 * address of the handle's map layer — layer 0 of the stack (0: no map; does not synchronise — po_set_map_occupancy_device / po_set_map_stack_occupancy_device with
 * an unchanged size and layer count must leave it where it is); "map_layers" = M, the number of layers the handle holds (0: no map; does not synchronise); "fixed_length_used" = 1 when the last solve ran the
 * length-specialised kernels, 0 when it ran the generic ones (does not synchronise); "fixed_classes_used" = how many paths of the last solve the constant-class Newton
 * kernels took (0: it did not run them), "fixed_classes_flag:<b>" = whether they took path b of it (1 yes, 0 no, -1 it did not run them; b outside the last batch:
 * PO_ERR_INVALID), "newton_list_ok" = 1 when the work lists of the second sliced Newton launch are what the sort promises — every parked path exactly once, keys
 * descending, ties in path order, and with the constant-class kernels each path on the list of the kernel its flag names (0 not, -1 not sliced); "dp_waves_used" = 8 or 1, the waves per instance of the handle's last DP lattice
 * search — po_dp_search_batch* or the search inside po_plan_batch* (0: none yet; does not synchronise): one wave above 512 instances, under "dp_one_wave", and when
 * the eight-wave reduction scratch does not fit in LDS beside the spline; "smooth_variant_used" = 100 * kind + 10 * waves + WPE, the instantiation of the smoothing kernel
 * that the handle's last po_smooth_batch* call launched: kind 0 .. 2, 1 / 4 / 8 waves per QP, WPE the occupancy bound it was compiled for (11, 42, 43 or 82; 0: no call
 * yet, and unchanged by a call that was refused before its launch; does not synchronise); "world_cells" = size_x * size_y of the handle's world grid (po_set_world_occupancy*; 0: none;
 * does not synchronise). */
int po_debug_get(po_handle h, const char *key, long long *value);

/* Host-pointer entry: H2D, solve, D2H, synchronous. */
int po_solve_batch(po_handle h, const po_batch_in *in, const po_batch_out *out);
/* Device-pointer entry: all pointers in `in`/`out` are device pointers; asynchronous on the stream. */
int po_solve_batch_device(po_handle h, const po_batch_in *in, const po_batch_out *out);
/* ---- post-solve step: PathOptimizer::optimizePath, src/path_optimizer/path_optimizer.cpp:183-200 ----
 * Upload the obstacle-distance layer (host pointer in `map->distance`) to the handle's device; kept until replaced. */
int po_set_map(po_handle h, const po_map *map);
/* ---- the obstacle-distance layer from an occupancy image, on the device (csrc/po_edt.hip) ----
 * What a planner has is an occupancy image; the reference's callers turn it into the layer on the host (src/test/path_optimizer_benchmark.cpp:38-43, demo.cpp:108):
 *     cv::distanceTransform(binary, distance, CV_DIST_L2, CV_DIST_MASK_PRECISE);  distance *= resolution;
 * The entries below compute exactly that layer, the EXACT Euclidean distance transform:
 *     d2(i, j)   = min over occupied cells (p, q) of (i - p)^2 + (j - q)^2                 (exact integer)
 *     dist(i, j) = float32(sqrt(double(d2(i, j)))) * float32(resolution)                    (correctly rounded root, one float32 multiply; occupied cells: +0.0f)
 * a function of exact integers: results are bit-identical to that definition, not merely close to it.
 * An image WITHOUT any occupied cell has no distance; OpenCV's answer there is an artefact of its table initialisation that nothing in the reference pins.  This
 * library's own choice: every cell gets float32(sqrt(double(size_x^2 + size_y^2))) * float32(resolution) — farther than any cell of the map can be from an
 * obstacle inside it, and finite, so the bilinear sampler stays finite.
 * `cells` is unsigned char, 0 = occupied, anything else free (cv::distanceTransform's convention, the reference's OCCUPY = 0), in po_map's layout:
 * [size_y][size_x] in memory, x contiguous, image after image for a batch; layer(i, j) = image(i, j).
 * Limits: 1 <= size_x, size_y <= 4096 and M <= 65535; beyond: PO_ERR_UNSUPPORTED.  Deterministic: integers and one rounding per cell, no atomics. */
typedef struct po_occupancy {
    const unsigned char *cells;  /* [M][size_y][size_x], 0 = occupied */
    int    size_x, size_y;
    double resolution, pos_x, pos_y;  /* as po_map (the raw transform reads resolution only) */
} po_occupancy;
/* The raw transform: M images of one size in, M float layers [M][size_y][size_x] out; the handle's map is not touched. */
int po_distance_map_batch(po_handle h, int M, const po_occupancy *occ, float *distance);         /* host pointers, synchronous */
int po_distance_map_batch_device(po_handle h, int M, const po_occupancy *occ, float *distance);  /* device pointers, on the stream */
/* Build the handle's map from ONE image: what po_set_map does, minus the host transform.  Afterwards the handle's map is indistinguishable from one installed by
 * po_set_map with the same layer.  Host entry: uploads 1 byte per cell, synchronous.  Device entry: `occ->cells` is a device pointer and the transform is enqueued on
 * the handle's stream, straight into the handle's map buffer: with the size the handle already holds it allocates nothing and does not synchronise, so a per-cycle
 * refresh followed by po_plan_batch_device is ordered by the stream alone (the image must stay valid until the stream has passed the call).  When a buffer has to
 * grow, the entry first synchronises the stream — everything enqueued earlier that reads the old buffer has finished — and only then releases it. */
int po_set_map_occupancy(po_handle h, const po_occupancy *occ);
int po_set_map_occupancy_device(po_handle h, const po_occupancy *occ);
/* Read the handle's current map back: geometry into *geometry_out (its `distance` is set to NULL) and, when distance_or_null is given, the layer
 * [size_y][size_x] into that host buffer.  Synchronous.  PO_ERR_INVALID when no map is set. */
int po_get_map(po_handle h, po_map *geometry_out, float *distance_or_null);
/* ---- per-instance maps: a STACK of layers and an ASSIGNMENT of instances to layers ----
 * A handle holds M >= 1 layers of one size_x, size_y and resolution (what po_distance_map_batch produces), each with its own map-centre position, and optionally a
 * table layer_of[n] that says which layer instance b of a batch reads.
 *   Single-map entries.  po_set_map and po_set_map_occupancy* install a stack with M = 1.  po_get_map, po_map_sample and po_debug_get "map_ptr" mean layer 0.
 *   Reading the assignment.  With no assignment every instance reads layer 0.  With an assignment of length n, instance b of ANY map-reading batch entry
 *     (po_bounds_batch*, po_dp_search_batch*, po_smooth_batch* with PO_SMOOTH_TENSION, po_postcheck_batch*, po_densify_batch*, and every map stage inside
 *     po_plan_batch*) reads layer layer_of[b].  A batch with B > n returns PO_ERR_INVALID.
 *   Validation.  po_set_map_assignment (host pointer) checks the table: any value outside [0, M) returns PO_ERR_INVALID and leaves the handle unchanged (the previous
 *     table stays in force); so does a table given before any map.  po_set_map_assignment_device cannot look at the table: every kernel clamps the index into
 *     [0, M - 1] where it reads it, so a bad table selects a wrong layer, never an address outside the stack.
 *   Lifetime.  An install that changes M clears the assignment; an install with the same M keeps it (a per-cycle refresh of M local grids does not re-send the table).
 *     n = 0 or layer_of = NULL clears it.
 *   Stack entries.  `layers->distance` / `occ->cells` hold M layers / images [M][size_y][size_x], one after the other; pos_xy is [M][2], the centre (x, y) of each
 *     layer, or NULL = every layer at layers->pos_x / pos_y (occ->pos_x / pos_y).  po_set_map_stack and po_set_map_stack_occupancy take host pointers and are
 *     synchronous.  po_set_map_stack_occupancy_device: `occ->cells` AND pos_xy are device pointers and everything is enqueued on the handle's stream (both must stay
 *     valid until the stream has passed the call); it keeps the contract of po_set_map_occupancy_device — with the M and size the handle already holds it allocates
 *     nothing and does not synchronise, and "map_ptr" stays where it is; when a block has to grow it synchronises the stream first.  The layers are bit for bit
 *     what po_distance_map_batch returns for the same images.
 *   Limits: those of po_distance_map_batch — 1 .. 4096 cells per side, M <= 65535, beyond: PO_ERR_UNSUPPORTED (po_set_map_stack too).
 *   po_get_map_layer / po_map_sample_layer: po_get_map / po_map_sample for layer k; k outside [0, M): PO_ERR_INVALID. */
int po_set_map_stack(po_handle h, int M, const po_map *layers, const double *pos_xy);                      /* host pointers, synchronous */
int po_set_map_stack_occupancy(po_handle h, int M, const po_occupancy *occ, const double *pos_xy);         /* host pointers, synchronous */
int po_set_map_stack_occupancy_device(po_handle h, int M, const po_occupancy *occ, const double *pos_xy);  /* cells and pos_xy are device pointers; on the stream */
int po_set_map_assignment(po_handle h, int n, const int *layer_of);          /* host pointer; n = 0 or NULL clears */
int po_set_map_assignment_device(po_handle h, int n, const int *layer_of);   /* device pointer, copied on the stream */
int po_get_map_layer(po_handle h, int k, po_map *geometry_out, float *distance_or_null);
int po_map_sample_layer(po_handle h, int k, int n, const double *xy, double *dist, int *inside);
/* ---- the stack from per-layer OBSTACLE LISTS, rasterised on the device (csrc/po_raster.hip) ----
 * A planner does not hold M images: it holds one static grid and, per hypothesis or vehicle, a short list of detected objects.  The entries below turn M such
 * lists into the M occupancy images po_distance_map_batch reads ([M][size_y][size_x], 0 = occupied, 255 = free) — and, for the stack entries, on into the M distance
 * layers — without the images ever existing on the host: a layer costs 136 bytes per obstacle over PCIe instead of one byte per cell.
 * Definition (the bar is BIT equality, as for the distance transform).  The centre of cell (i, j) of layer k is grid_map's getPositionFromIndex,
 *     px = (pos_x[k] + (0.5 * (size_x * resolution) - 0.5 * resolution)) + resolution * (-i),    py likewise with size_y, pos_y[k] and j,
 * evaluated in IEEE double, one rounding per operation, nothing contracted.  A cell is occupied when its base cell is 0 (if a base is given) or when its centre is
 * covered by any obstacle of the layer:
 *   DISC   dx = px - v[0], dy = py - v[1]:  dx * dx + dy * dy <= v[2] * v[2]   (the boundary is inclusive);
 *   POLY   the centre lies in the closed bounding box of the vertices (exact min / max) AND the cross products (bx - ax) * (py - ay) - (by - ay) * (px - ax) of
 *          all edges (a -> b, the last edge closing back to vertex 0) are all >= 0 or all <= 0.  Convex polygons of either orientation; the bounding-box clause
 *          keeps a degenerate (collinear) polygon a segment.  A NON-convex polygon gets what this predicate says (its convex kernel, roughly): not supported.
 * A comparison with a NaN is false; an obstacle with an unknown kind, a POLY with n_verts < 3, or a NaN among the values its kind reads (DISC: v[0 .. 2]; POLY:
 * the first 2 n_verts) covers nothing.  A layer without any occupied cell then falls under the distance transform's no-obstacle rule, unchanged.
 * Host entries validate everything before they touch the handle — PO_ERR_INVALID, handle unchanged, for: first[0] != 0, first[] not non-decreasing, first[M] > n_obs;
 * an unknown kind; n_verts outside 3 .. PO_OBS_MAX_VERTS for a POLY; a negative or non-finite radius; a non-finite coordinate; base_count not in {0, 1, M};
 * base == NULL with base_count != 0.  n_obs = 0 and empty layers are valid.  Device entries cannot look at the lists: they read n_verts clamped into [0, 8] and first[]
 * clamped into [0, n_obs], so a bad list rasterises wrongly but never reads outside obs.  Limits: those of po_distance_map_batch, beyond: PO_ERR_UNSUPPORTED.
 * pos_xy is [M][2] or NULL (every layer at lists->pos_x / pos_y), exactly as in po_set_map_stack_occupancy*.
 * po_set_map_stack_obstacles* = the rasteriser into an image block the handle owns, then the very sequence of po_set_map_stack_occupancy_device.  The device entry keeps
 * that entry's contract word for word: with the M and size the handle already holds it allocates nothing and does not synchronise, and "map_ptr" stays where it is;
 * when a block has to grow it synchronises the stream first.  The assignment's lifetime rules apply unchanged.  The host entry uploads obs, first, pos_xy and the
 * base only.  Every pointer given to a device entry (those inside the struct too) is a device pointer and must stay valid until the stream has passed the call. */
#define PO_OBS_DISC 0
#define PO_OBS_POLY 1
#define PO_OBS_MAX_VERTS 8
typedef struct po_obstacle {
    int    kind;      /* PO_OBS_DISC / PO_OBS_POLY */
    int    n_verts;   /* POLY: 3 .. PO_OBS_MAX_VERTS; DISC: ignored */
    double v[16];     /* DISC: v[0], v[1] = centre (world frame), v[2] = radius >= 0.
                         POLY: (x, y) of vertex 0 .. n_verts-1, world frame, convex, either orientation */
} po_obstacle;        /* 136 bytes */
typedef struct po_obstacle_lists {
    const po_obstacle   *obs;     /* [n_obs] */
    const int           *first;   /* [M + 1], first[0] = 0, non-decreasing, first[M] <= n_obs:
                                     layer k owns obs[first[k] .. first[k+1]) */
    int                  n_obs;
    const unsigned char *base;    /* NULL = every cell free; else base_count images [size_y][size_x], 0 = occupied (po_occupancy's convention) */
    int                  base_count;  /* 0, 1 (one image shared by every layer, cell (i,j) -> cell (i,j)) or M.  A shared base IGNORES pos_xy: it means the
                                         same thing in every layer only when all layers have one centre.  The position-aware form of a static grid is the
                                         world grid (po_set_world_occupancy, po_scene.use_world). */
    int    size_x, size_y;
    double resolution, pos_x, pos_y;  /* as po_occupancy */
} po_obstacle_lists;
int po_rasterize_batch(po_handle h, int M, const po_obstacle_lists *lists, const double *pos_xy, unsigned char *cells_out);         /* host pointers, synchronous */
int po_rasterize_batch_device(po_handle h, int M, const po_obstacle_lists *lists, const double *pos_xy, unsigned char *cells_out);  /* device pointers, on the stream */
int po_set_map_stack_obstacles(po_handle h, int M, const po_obstacle_lists *lists, const double *pos_xy);                           /* host pointers, synchronous */
int po_set_map_stack_obstacles_device(po_handle h, int M, const po_obstacle_lists *lists, const double *pos_xy);                    /* device pointers, on the stream */
/* ---- the STATIC WORLD of the stack: a world grid on the handle and polygon rings (csrc/po_scene.hip) ----
 * Two more sources of occupied cells in front of the distance transform.  (1) What a planner holds of its site is ONE large static occupancy grid; each layer of
 * the stack is a window into it at pos_xy[k].  (2) The other half of what perception and HD maps deliver is a boundary: a free-space or drivable-area ring of tens to
 * hundreds of vertices, non-convex, with everything outside it not drivable — and non-convex blobs such as building footprints.
 *
 * The world grid.  One static occupancy image of the whole site, kept on the handle's device until replaced.  Layout and convention of po_occupancy (0 = occupied,
 * [size_y][size_x], x contiguous, centre pos_x / pos_y, its OWN resolution, which need not be the layers').  outside_occupied: what a layer cell whose centre falls
 * outside the world is (0 = free, 1 = occupied).  world == NULL clears it.  The handle owns its copy (a grow-only block; when it has to grow, the stream is
 * synchronised first): the caller's image may be reused as soon as the stream has passed the call (host entry: on return).  PO_ERR_INVALID: a NULL image, a size
 * below 1, a resolution that is not positive and finite, a non-finite centre, outside_occupied not in {0, 1}.  Limits: 1 .. 16384 cells per side; beyond:
 * PO_ERR_UNSUPPORTED.  po_debug_get "world_cells" returns size_x * size_y, or 0 when there is none.
 *
 * Definition (the bar is BIT equality, as for po_rasterize_batch).  The cell centre (px, py) of cell (i, j) of layer k is the one of po_rasterize_batch, unchanged.
 * A cell is occupied when any of the following five clauses holds.  Every operation is one rounded IEEE double operation, nothing is contracted, and a comparison
 * with a NaN is false.
 *   base, obstacles   as po_rasterize_batch (DISC, POLY), on scene->lists.
 *   world (only with use_world).  The world has wsx, wsy, wres, wpx, wpy;  lx = (double)wsx * wres, ly likewise.  This is grid_map's isInside and
 *          getIndexFromPosition:  tx = -((px - wpx) - 0.5 * lx), ty likewise; the centre is inside <=> tx >= 0 && ty >= 0 && tx < lx && ty < ly;
 *          ix = (int)(-(((px - 0.5 * lx) - wpx) / wres)), iy likewise (the conversion truncates).  Inside and 0 <= ix < wsx && 0 <= iy < wsy:
 *          occupied <=> world[iy][ix] == 0.  Otherwise: occupied <=> outside_occupied.
 *   SOLID rings       some SOLID ring the layer owns (shared or its own) CONTAINS the centre.
 *   FREE rings        the layer owns at least one FREE ring and none of them CONTAINS the centre.
 * CONTAINS is the even-odd rule with the cross product POLY uses, for a ring with n >= 3 vertices.  For every edge a -> b (the last one closing back to vertex 0):
 *          straddles = (ay > py) != (by > py);   t = (bx - ax) * (py - ay) - (by - ay) * (px - ax);   right = (by > ay) ? (t > 0) : (t < 0).
 * The ring contains the centre when the number of edges with straddles && right is odd.  Consequences: orientation does not matter; of an axis-aligned box the low
 * edges belong to it and the high edges do not; a self-intersecting ring gets even-odd filling; a horizontal edge never counts.  Holes are not a ring attribute: use
 * a FREE outer ring plus SOLID islands.
 * Device entries cannot look at the arrays, so they read them clamped: start[] into [0, n_verts]; n_shared and first[] into [0, n_rings]; a ring with fewer than 3
 * vertices is ignored and does not count as a FREE ring of the layer; a ring with more than PO_RING_MAX_VERTS is read as its first PO_RING_MAX_VERTS vertices, with
 * the closing edge from the last of them to vertex 0; a ring whose flag is neither 0 nor 1 is ignored; first == NULL means no layer owns rings of its own.  A bad
 * table rasterises wrongly.  It never reads outside verts, start, flags or the world block.
 * Host entries refuse with PO_ERR_INVALID, before they touch the handle: a table that breaks an inequality stated at po_rings; a ring with fewer than 3 or more than
 * PO_RING_MAX_VERTS vertices; a non-finite vertex; an unknown flag; first == NULL with n_shared != n_rings; anything po_rasterize_batch refuses.  Every entry refuses
 * negative counts, a NULL array with a positive count, use_world not in {0, 1}, and use_world without a world on the handle.
 * A scene with n_rings == 0 and use_world == 0 gives the bytes of po_rasterize_batch on scene->lists.
 * po_set_map_stack_scene* = the scene rasteriser into the image block the handle owns, then the very sequence of po_set_map_stack_occupancy_device; the device entry
 * keeps that entry's contract word for word (with the M and size the handle already holds it allocates nothing and does not synchronise, and "map_ptr" stays where it
 * is; the same M keeps the assignment; a block that has to grow does so behind a synchronisation of the stream). */
int po_set_world_occupancy(po_handle h, const po_occupancy *world, int outside_occupied);         /* host pointer, synchronous */
int po_set_world_occupancy_device(po_handle h, const po_occupancy *world, int outside_occupied);  /* device pointer; copied into the handle's block on the stream */
#define PO_WORLD_MAX_SIDE 16384
#define PO_RING_SOLID 0      /* the ring's interior is occupied */
#define PO_RING_FREE  1      /* free space: a layer that owns FREE rings is occupied wherever none of them contains the cell */
#define PO_RING_MAX_VERTS 4096
typedef struct po_rings {
    const double *verts;   /* [n_verts][2]: x, y, world frame */
    const int    *start;   /* [n_rings + 1], start[0] = 0, non-decreasing, start[n_rings] <= n_verts: ring r owns verts[start[r] .. start[r+1]) */
    const int    *flags;   /* [n_rings]: PO_RING_SOLID / PO_RING_FREE */
    int n_rings, n_verts;
    int n_shared;          /* rings [0, n_shared) belong to EVERY layer (the static world: drivable area, buildings) */
    const int    *first;   /* NULL (then n_shared == n_rings) or [M + 1], first[0] == n_shared, non-decreasing, first[M] <= n_rings:
                              layer k also owns rings [first[k], first[k+1]) */
} po_rings;
typedef struct po_scene {
    po_obstacle_lists lists;   /* exactly as today: layer geometry, discs / convex polygons, base */
    po_rings          rings;   /* n_rings == 0: none (the other fields are not looked at) */
    int               use_world;  /* 1: the handle's world grid contributes; PO_ERR_INVALID when none is installed */
} po_scene;
int po_rasterize_scene_batch(po_handle h, int M, const po_scene *scene, const double *pos_xy, unsigned char *cells_out);         /* host pointers, synchronous */
int po_rasterize_scene_batch_device(po_handle h, int M, const po_scene *scene, const double *pos_xy, unsigned char *cells_out);  /* device pointers, on the stream */
int po_set_map_stack_scene(po_handle h, int M, const po_scene *scene, const double *pos_xy);                                     /* host pointers, synchronous */
int po_set_map_stack_scene_device(po_handle h, int M, const po_scene *scene, const double *pos_xy);                              /* device pointers, on the stream */
/* For every path: walk the optimised states in order and stop at the first state that fails
 * CollisionChecker::isSingleStateCollisionFreeImproved (src/tools/collision_checker.cpp:42-59: bounding circle, then the
 * six footprint circles of src/tools/car_geometry.cpp:38-72; outside the map = collision).
 *   n_valid[b] = number of states kept (the reference erases from the colliding state on);
 *   ok[b]      = what optimizePath returns: 0 if the QP was not solved (info[b].status != PO_STATUS_SOLVED),
 *                1 if no state collides, else (s of the last kept state >= 20 m); 0 if the first state collides.
 * `states`/`info` are the outputs of po_solve_batch* ([B][N][5], [B]); n_points as in po_batch_in (or NULL).
 * With params.enable_collision_check == 0 every solved path is kept whole.  Host-pointer and device-pointer entries. */
int po_postcheck_batch(po_handle h, int B, int N, const int *n_points, const double *states, const po_info *info,
                       int *n_valid, int *ok);
int po_postcheck_batch_device(po_handle h, int B, int N, const int *n_points, const double *states, const po_info *info,
                              int *n_valid, int *ok);
/* The other output branch of optimizePath (FLAGS_enable_raw_output = false, path_optimizer.cpp:201-226): x(s), y(s) splines through the
 * solved states, sampled every FLAGS_output_spacing with heading and curvature from the spline, each sample collision-checked; the walk
 * stops at the first colliding sample.  out_states [B][M][5]; n_out[b] samples kept; ok[b] as po_postcheck_batch (0 for an unsolved QP;
 * the reference dereferences back() of an empty vector when the very first sample collides: reported as ok = 0, n_out = 0);
 * n_out[b] = -2 (and ok[b] = 0) when M is too small.  An output_spacing that is not positive (NaN included): PO_ERR_INVALID, no kernel launched, outputs not written. */
int po_densify_batch(po_handle h, int B, int N, const int *n_points, const double *states, const po_info *info, int M, double *out_states, int *n_out,
                     int *ok);
int po_densify_batch_device(po_handle h, int B, int N, const int *n_points, const double *states, const po_info *info, int M, double *out_states,
                            int *n_out, int *ok);
/* ---- corridor-bounds producer: ReferencePath::updateBounds -> ReferencePathImpl::updateBoundsImproved,
 * src/data_struct/reference_path_impl.cpp:142-201 (+ getApproxState :121-140, getClearanceWithDirectionStrict :283-472 with
 * FLAGS_enable_simple_boundary_decision = true as shipped, tk::spline src/tools/spline.cpp).  Needs po_set_map.
 * FLAGS_enable_simple_boundary_decision (src/config/planning_flags.cpp:84): no po_params field, because it has no effect in the reference either — the branch it
 * selects in getClearanceWithDirectionStrict (:322) also requires is_original_spline_set, and ReferencePath::setOriginalSpline (reference_path.cpp:95) has no caller
 * anywhere in the reference: the reference-compiled producer returns bit-identical bounds for both values (tests/test_bounds.py).  Only a caller that patches the
 * reference to CALL setOriginalSpline and clears the flag gets bounds this entry does not produce; such a caller keeps its CPU producer and hands po_batch_in.bounds over.
 * Inputs per path: the N reference states (x, y, heading, s) and the K knots (s, x, y) the path's x(s) / y(s) splines were set
 * from (tk::spline::set_points, natural boundary conditions — what ReferencePath::setSpline receives).
 * Outputs: bounds [B][N][4][2] = (lb, ub) of the four covering circles, directly consumable as po_batch_in.bounds, and
 * n_valid[b] = number of states kept (the reference stops at the first blocked state and truncates the reference there);
 * rows >= n_valid[b] are zero.  n_valid is directly consumable as po_batch_in.n_points (when >= 2). */
typedef struct po_bounds_in {
    int B, N, K;                                   /* paths, reference states per path (stride), knots per path (stride) */
    const double *ref_x, *ref_y, *ref_z, *ref_s;   /* [B][N] */
    const int    *n_points;                        /* optional [B]: states of each path (<= N) */
    const double *knot_s, *knot_x, *knot_y;        /* [B][K], knot_s strictly increasing */
    const int    *n_knots;                         /* optional [B]: knots of each path (3 <= n_knots[b] <= K) */
} po_bounds_in;
int po_bounds_batch(po_handle h, const po_bounds_in *in, double *bounds, int *n_valid);        /* host pointers, synchronous  */
int po_bounds_batch_device(po_handle h, const po_bounds_in *in, double *bounds, int *n_valid); /* device pointers, on the stream */

/* ---- reference-smoothing QPs: the three other places where the reference hands a chain-structured QP to
 * OsqpEigen with the same call pattern as the hot path (setHessianMatrix ... initSolver, solve):
 *   PO_SMOOTH_TENSION2  TensionSmoother2::osqpSmooth       src/reference_path_smoother/tension_smoother_2.cpp:163-301
 *                       (FLAGS_smoothing_method = "TENSION2", FLAGS_tension_solver = "OSQP": the shipped defaults)
 *   PO_SMOOTH_TENSION   TensionSmoother::osqpSmooth        src/reference_path_smoother/tension_smoother.cpp:186-314  (needs po_set_map)
 *   PO_SMOOTH_POST      ReferencePathSmoother::postSmooth  src/reference_path_smoother/reference_path_smoother.cpp:534-644 (the QP; the
 *                       re-projection onto the spline that follows it stays with the caller)
 * One batch = B independent instances with up to P points each (arrays [B][P], ragged through n_points).
 *   TENSION2 / TENSION inputs: x, y, angle, k, s = the five lists segmentRawReference produces (reference_path_smoother.cpp:50-91);
 *       outputs: out_x, out_y, out_s = result_x_list, result_y_list, result_s_list (s = running chord length of the result).
 *   POST inputs: s = layers_s_list_, lb / ub = layers_bounds_ (.first / .second), l0[b] = vehicle_l_wrt_smoothed_ref_;
 *       x, y, angle, k unused (may be NULL); output: out_x[b][i] = QPSolution(i), the lateral offset of layer i; out_y / out_s unused.
 * info[b].status == PO_STATUS_SOLVED <=> the reference's `solver.solve()` returned true; raw (optional) = the whole QP solution in
 * the REFERENCE variable order, [B][n_max] with n_max = po_smooth_dims(kind, P).  OSQP settings come from the handle's po_params
 * (the reference runs the smoothers at OSQP's default eps_abs = eps_rel = 1e-3; create the handle accordingly to mirror that).
 * Fewer points than the reference accepts (TENSION*: 3, POST: 4, reference_path_smoother.cpp:536) -> PO_ERR_INVALID.  That is judged on P; n_points is
 * not screened by either entry (the device entry cannot read it): an instance whose n_points[b] is below that minimum or above P comes back with
 * info[b].status == PO_STATUS_UNSOLVED and zero rows of out_x / out_y / out_s (raw[b] is not written: do not read it for such an instance), the other instances are unaffected.
 * A P whose QP does not fit the on-chip tile -> PO_ERR_UNSUPPORTED, nothing written (the admissible P are not one interval: the footprint steps with the
 * layout of the substitution; the largest are 344 / 349 / 473 for TENSION2 / TENSION / POST). */
enum { PO_SMOOTH_TENSION2 = 0, PO_SMOOTH_TENSION = 1, PO_SMOOTH_POST = 2 };
typedef struct po_smooth_in {
    int kind, B, P;
    const int    *n_points;            /* optional [B] */
    const double *x, *y, *angle, *k;   /* [B][P] */
    const double *s;                   /* [B][P] */
    const double *lb, *ub;             /* [B][P]  POST only */
    const double *l0;                  /* [B]     POST only */
} po_smooth_in;
typedef struct po_smooth_out {
    double  *x, *y, *s;   /* [B][P] (y, s may be NULL for POST) */
    po_info *info;        /* [B] */
    double  *raw;         /* optional [B][n_max] */
} po_smooth_out;
/* QP dimensions as the reference sets them (tension_smoother_2.cpp:177-178, tension_smoother.cpp:201-202, reference_path_smoother.cpp:544-545) */
int po_smooth_dims(int kind, int P, int *n, int *m);
int po_smooth_batch(po_handle h, const po_smooth_in *in, const po_smooth_out *out);        /* host pointers, synchronous  */
int po_smooth_batch_device(po_handle h, const po_smooth_in *in, const po_smooth_out *out); /* device pointers, on the stream */

/* ---- reference re-sampling, limits and the DP lattice search ----
 * A batch of planar splines x(s), y(s) (tk::spline, natural boundary conditions) given by the knots they were set from, plus the arc
 * length the reference attaches to them (ReferencePath::getLength(), i.e. max_s_). */
typedef struct po_spline_in {
    int B, K;                                /* instances, knots per instance (stride) */
    const double *knot_s, *knot_x, *knot_y;  /* [B][K], knot_s strictly increasing */
    const int    *n_knots;                   /* optional [B]: 3 <= n_knots[b] <= K */
    const double *length;                    /* [B]: max_s_ */
} po_spline_in;
/* ReferencePathImpl::buildReferenceFromSpline (src/data_struct/reference_path_impl.cpp:474-499): walk the spline from s = 0 while
 * s <= length with the curvature-adaptive step (FLAGS_enable_dynamic_segmentation; |k| >= 0.2 -> delta_s_smaller, |k| <= 0.08 ->
 * delta_s_larger, linear in between) and emit State{x, y, heading, k, s} (getHeading / getCurvature, src/tools/tools.cpp:34-47).
 * Outputs [B][N] (directly consumable as po_batch_in.ref_* / po_bounds_in.ref_*) and n_points[b]; n_points[b] = -1 when the reference
 * returns false (length <= 0) and -2 when more than N states would be produced (raise N); rows beyond n_points are zero. */
int po_resample_batch(po_handle h, const po_spline_in *in, double delta_s_smaller, double delta_s_larger, int N, double *ref_x, double *ref_y,
                      double *ref_z, double *ref_k, double *ref_s, int *n_points);
int po_resample_batch_device(po_handle h, const po_spline_in *in, double delta_s_smaller, double delta_s_larger, int N, double *ref_x,
                             double *ref_y, double *ref_z, double *ref_k, double *ref_s, int *n_points);
/* ReferencePathImpl::updateLimits (reference_path_impl.cpp:203-235), the branch the KPC formulation uses (reference states given
 * directly, with speed v and acceleration a): max_k = sqrt((mu g)^2 - a^2) / v^2, max_kp = max_curvature_rate / v, DBL_MAX for
 * v <= 1e-4.  Outputs [B][N] are directly consumable as po_batch_in.max_k / max_kp. */
int po_limits_batch(po_handle h, int B, int N, const int *n_points, const double *v, const double *a, double *max_k, double *max_kp);
int po_limits_batch_device(po_handle h, int B, int N, const int *n_points, const double *v, const double *a, double *max_k, double *max_kp);
/* ReferencePathSmoother::graphSearchDp (src/reference_path_smoother/reference_path_smoother.cpp:147-300, cost :110-145): project the
 * vehicle onto the spline (findClosestPoint, tools.cpp:71-112), lay out layers every FLAGS_search_longitudial_spacing, sample each at
 * lateral offsets -range..range every FLAGS_search_lateral_spacing against the obstacle map (po_set_map), run the layer-by-layer
 * min-cost recursion and walk back from the cheapest node of the last reachable layer widening each node's rough corridor in 0.2 m
 * steps.  start [B][3] = start_state (x, y, heading).  Outputs, [B][L]: layer_s = layers_s_list_, lb / ub = layers_bounds_
 * (.first / .second); l0[b] = vehicle_l_wrt_smoothed_ref_; n_layers[b] = layers kept, -1 when the reference returns false (vehicle
 * further than the lateral range from the spline), -2 when more than L layers are needed.  These are the inputs of PO_SMOOTH_POST.
 * One wave carries the lateral samples of a layer: search_lateral_range, search_long_spacing or search_lat_spacing that is not positive (NaN included), or
 * 2 * search_lateral_range / search_lat_spacing + 1 > 64, returns PO_ERR_UNSUPPORTED before any kernel is launched (the outputs are not written).  The number of
 * samples is the reference's running sum from -range in steps of the spacing while <= range, at most 64. */
int po_dp_search_batch(po_handle h, const po_spline_in *in, const double *start, int L, double *layer_s, double *lb, double *ub, double *l0,
                       int *n_layers);
int po_dp_search_batch_device(po_handle h, const po_spline_in *in, const double *start, int L, double *layer_s, double *lb, double *ub,
                              double *l0, int *n_layers);

/* ---- the remaining glue stages of PathOptimizer::solve, device-pointer entries (each is one kernel on the handle's stream) ----
 * ReferencePathSmoother::bSpline (reference_path_smoother.cpp:495-532): dense samples x_list_, y_list_, s_list_ [B][M] of the clamped
 * B-spline whose control points are the input points (tinyspline, a library that is NOT in /root/reference: restated, parity unpinned);
 * n_samples[b] = -1 for fewer than 4 points ("Few reference points."), -2 if M is too small. */
int po_bspline_batch_device(po_handle h, int B, int W, const int *n_way, const double *way_x, const double *way_y, int M, double *x, double *y, double *s,
                            int *n_samples);
/* ReferencePathSmoother::segmentRawReference (:50-91): the spline through the dense lists (raw->knot_*, raw->n_knots; raw->length unused)
 * sampled at 1 m stations: x, y, s, angle, k [B][P] = the five inputs of PO_SMOOTH_TENSION2 / PO_SMOOTH_TENSION; n_points as above. */
int po_segment_raw_batch_device(po_handle h, const po_spline_in *raw, int P, double *x, double *y, double *s, double *angle, double *k, int *n_points);
/* The tail of ReferencePathSmoother::postSmooth (:568-590): layer i moves to xs(s_i) + l_i (cos, sin)(heading + pi/2); x, y, s [B][L] are the
 * knots of the re-fitted spline (s = running chord length), length[b] = s.back() (may be NULL). */
int po_post_project_batch_device(po_handle h, const po_spline_in *spline, int L, const int *n_layers, const double *layer_s, const double *offsets, double *x,
                                 double *y, double *s, double *length);
/* PathOptimizer::segmentSmoothedPath up to the re-sampling (path_optimizer.cpp:119-169): init [B][3] = initial_offset,
 * initial_heading_error, length after the goal trim; ok[b] = 0 where the reference returns false (empty path, heading error > 75 deg).
 * start [B][start_stride] = x, y, heading, ...; goal [B][goal_stride] = x, y, ... */
int po_segment_init_batch_device(po_handle h, const po_spline_in *spline, const double *start, int start_stride, const double *goal, int goal_stride,
                                 double *init, int *ok);

/* ---- PathOptimizer::solve for a batch of planning instances (path_optimizer.cpp:40-85): bSpline -> TensionSmoother2 -> graphSearchDp ->
 * postSmooth -> segmentSmoothedPath (goal trim, buildReferenceFromSpline(0.15, FLAGS_output_spacing = 0.3), updateBounds) -> KP QP ->
 * collision check, every stage on the device, chained through HBM (one D2H of 3 ints per instance in the middle to group the QPs by
 * keep_control_steps_).  Needs po_set_map.  The shipped flag defaults are assumed (smoothing_method TENSION2, tension_solver OSQP,
 * optimization_method KP, enable_raw_output, enable_collision_check from po_params); OSQP settings from po_params for all three QPs.
 *   way_x / way_y [B][W]: reference_points (solve() reads only x and y); start [B][4] = start_state x, y, heading, k; goal [B][3].
 *   states [B][N][5] = final_path (x, y, heading, k, s), n_states[b] its size, ok[b] = the bool solve() returns;
 *   stage[b] (optional) = 0 or the stage that made it return false: 1 too few points / B-spline, 2 tension smoothing QP, 3 graph search,
 *   4 post smoothing, 5 segmentation (heading error > 75 deg), 6 reference blocked at its start, 7 path QP, 8 collision check (states
 *   hold the truncated path), 9 capacity (N / max_length too small or the QP does not fit the on-chip tile).
 *   max_length: upper bound of the waypoint polyline lengths (sizes the intermediate buffers); <= 0: computed from the waypoints
 *   (host-pointer entry only).
 *   Limits (the reference has none): max_length up to 316 m — the tension smoothing QP over ceil(max_length) + 6 points must fit the on-chip tile, which every size
 *   up to 322 points does (TENSION2; some sizes up to 344 fit too; TENSION: 349); the spline stages, which keep 120 x knots bytes in LDS, would allow 546.
 *   Beyond that the call returns PO_ERR_UNSUPPORTED for the whole batch, from the smoothing stage; the path QP of an instance must fit the on-chip tile — at the default 0.15 ... 0.3 m
 *   re-sampling that is a route of roughly 75 m (keep_control_steps_ <= 4: N <= 512) to 150 m; longer instances come back with stage 9, the others are unaffected.
 *   The lattice search inside the chain has room for max(ceil((max_length + 3) / search_long_spacing), 14) + 8 layers, as long as the post-smoothing QP over that
 *   many layers fits the on-chip tile (473 layers at most): an instance that needs more (at search_long_spacing = 0.5 a route beyond about 230 m) comes back with
 *   stage 9 as well, the others are unaffected.
 *   Settings: the search refuses its settings as po_dp_search_batch* does (PO_ERR_UNSUPPORTED for the call).  With enable_raw_output the reference is re-sampled at
 *   0.15 m / output_spacing: an output_spacing below 0.15, not positive or NaN is the reference's CHECK_LE(delta_s_smaller, delta_s_larger) and returns
 *   PO_ERR_INVALID for the call — from the re-sampling stage, i.e. after the stages before it were enqueued; the outputs are unspecified then. */
typedef struct po_plan_in {
    int B, W;
    const int    *n_way;          /* optional [B] */
    const double *way_x, *way_y;  /* [B][W] */
    const double *start, *goal;   /* [B][4], [B][3] */
    double max_length;
    int N;                        /* rows of `states` per instance */
} po_plan_in;
typedef struct po_plan_out {
    double  *states;   /* [B][N][5] */
    int     *n_states; /* [B] */
    int     *ok;       /* [B] */
    int     *stage;    /* optional [B] */
    po_info *info;     /* optional [B]: the path QP */
} po_plan_out;
int po_plan_batch(po_handle h, const po_plan_in *in, const po_plan_out *out);         /* host pointers, synchronous */
int po_plan_batch_device(po_handle h, const po_plan_in *in, const po_plan_out *out);  /* device pointers; synchronises the stream once mid-way */

/* ---- score and select: B candidate paths -> eight features and a cost each, one winner per group, the winners gathered (csrc/po_select.hip) ----
 * The output side of "many hypotheses per call": po_plan_batch* leaves B paths in HBM; the caller wants one decision per vehicle.  A group is a contiguous range
 * of candidates (the variants of one vehicle); the call scores every candidate against the map layer it was planned on, picks the cheapest feasible one of each
 * group and copies the winners' rows out, so that G paths cross PCIe instead of B.  sel_states / sel_n have the layout of prev_states / prev_n: fed back unchanged
 * in the next cycle they give the hysteresis feature (distance to last cycle's choice) without leaving the device.  The reference has no such stage.
 *
 * Map access.  Candidate b reads the layer every map stage reads for instance b (the assignment of po_set_map_assignment*, else layer 0).  The call needs a map and
 * an assignment that covers B: PO_ERR_INVALID otherwise, as po_bounds_batch*.  The footprint is the six circles (cx_q, cy_q, cr_q) of the post-solve collision check
 * (CarGeometry from po_params: rr, rl, fr, fl, fm, rm); its bounding circle is not used.
 *
 * Definition (the bar is BIT equality).  Every operation is one rounded IEEE double operation in the order written, nothing contracted; a comparison with a NaN is
 * false; min(a, b) = b < a ? b : a; max(a, b) = b > a ? b : a.  n = n_states[b] clamped into [0, N] (N when NULL); row i = (x_i, y_i, z_i, k_i, s_i).
 *   Per state i < n:   cz = pcos(z_i), sz = psin(z_i) (include/po_pmath.h);  for q = 0 .. 5:  gx = (cx_q * cz - cy_q * sz) + x_i,  gy = (cx_q * sz + cy_q * cz) + y_i,
 *       c_iq = D(gx, gy) - cr_q with D = Map::getObstacleDistance on the candidate's layer (0 outside the map, so the clearance there is -cr_q);
 *       c_i = c_i0, then c_i = min(c_i, c_iq) for q = 1 .. 5;   t = d_safe - c_i, t = t > 0 ? t : 0, p_i = t * t;   e_i: below.
 *   Per interval i < n - 1, ds_i = s_{i+1} - s_i:
 *       T1_i = (0.5 * (k_i * k_i + k_{i+1} * k_{i+1})) * ds_i          T2_i = ds_i > 0 ? ((k_{i+1} - k_i) * (k_{i+1} - k_i)) / ds_i : 0
 *       T5_i = (0.5 * (p_i + p_{i+1})) * ds_i                          T7_i = (0.5 * (e_i + e_{i+1})) * ds_i
 *   The fold F(op, init, v):  64 partials P_t = init;  for i ascending P_{i mod 64} = op(P_{i mod 64}, v_i);  then for h = 32, 16, 8, 4, 2, 1: P_t = op(P_t, P_{t+h})
 *       for t < h;  the result is P_0.  It is fixed so that a path's features depend neither on the batch size nor on the path's position in the batch.
 *   Features:  0 LENGTH = s_{n-1}    1 CURV = F(+, +0.0, T1)    2 CURV_RATE = F(+, +0.0, T2)    3 KMAX = F(max, +0.0, |k_i|)    4 CLR_MIN = F(min, DBL_MAX, c_i)
 *       5 PROX = F(+, +0.0, T5)    6 GOAL = sqrt((x_{n-1} - gx) * (x_{n-1} - gx) + (y_{n-1} - gy) * (y_{n-1} - gy)) with (gx, gy) = goal[b][0 .. 1], 0 when goal is NULL
 *       7 DEV_PREV = F(+, +0.0, T7).   n = 0: LENGTH = GOAL = 0 (the folds give 0, 0, 0, DBL_MAX, 0, 0).
 *   e_i, the squared distance of state i to the previous path of the candidate's group g: np = prev_n[g] clamped into [0, Np] (Np when NULL), points (u_j, v_j) =
 *       columns 0 and 1 of rows j < np of prev_states[g].  e_i = 0 for every i when prev_states is NULL, Np = 0, np < 2 or the candidate is in no group.  Otherwise,
 *       for segment j = 0 .. np - 2:  dx = u_{j+1} - u_j, dy = v_{j+1} - v_j, px = x_i - u_j, py = y_i - v_j;  L2 = dx * dx + dy * dy, dot = px * dx + py * dy;
 *       t = L2 > 0 ? dot / L2 : 0, then t = t < 0 ? 0 : t, then t = t > 1 ? 1 : t;  qx = px - t * dx, qy = py - t * dy, D_j = qx * qx + qy * qy;
 *       e_i = D_0, then e_i = min(e_i, D_j) for j = 1 .. np - 2.  Np is not limited.
 *   Feasible <=> ok[b] != 0 (NULL: 1), n >= 2, every value of rows < n is finite, all eight features are finite, CLR_MIN >= min_clearance, KMAX <= max_kmax,
 *       GOAL <= max_goal_dist, and the cost below is finite.
 *   cost = (((((((w0 * f0 + w1 * f1) + w2 * f2) + w3 * f3) + w4 * f4) + w5 * f5) + w6 * f6) + w7 * f7) of a feasible candidate, +infinity otherwise.
 *   Selection: best[g] = the feasible candidate of group g with the smallest cost, the smallest index among equal costs; best_cost[g] its cost; n_feasible[g] how
 *       many are feasible; sel_n[g] = its n, rows < n of sel_states[g] are bitwise its rows and the rest are zero.  No feasible candidate (or an empty group):
 *       best = -1, best_cost = +infinity, n_feasible = 0, sel_n = 0, all rows zero.
 * Groups.  group_start[G + 1]: group g = candidates [group_start[g], group_start[g+1]).  The host entry validates the table — non-decreasing, group_start[0] >= 0,
 *   group_start[G] <= B, else PO_ERR_INVALID.  The device entry cannot: its kernels read gs'[0] = clamp(gs[0], 0, B), gs'[g+1] = clamp(max(gs[g+1], gs'[g]), 0, B)
 *   (a small launch ahead of the two kernels writes gs' into the handle's scratch), and n_states / prev_n clamped where they are read: a bad table selects wrong
 *   rows, never an address outside the buffers.  A candidate outside every group is scored and never selected; its e_i are 0.
 * Return codes.  PO_ERR_INVALID: a NULL handle, struct or required pointer (B > 0 and G > 0: states, group_start, best; sel_n when sel_states is given; goal needs
 *   goal_stride >= 2); a negative B, N, G; prev_states given with Np < 0; a non-finite weight; a NaN among d_safe, min_clearance, max_kmax, max_goal_dist; no map; an
 *   assignment shorter than B.  B = 0 or G = 0: PO_OK, nothing is launched and nothing is written — this is decided after the argument checks above and BEFORE
 *   the map and assignment rule, so an empty call is PO_OK on a handle without a map too.
 * `p` is a host pointer in both entries.  cost goes to a block the handle owns when out->cost is NULL (the selection reads it).  Deterministic: no atomics.
 * po_default_select_params: w = {1, 10, 10, 0, 0, 10, 5, 1}, d_safe = 0.5, min_clearance = 0, max_kmax = max_goal_dist = DBL_MAX — a starting point nobody has tuned. */
enum { PO_FEAT_LENGTH = 0, PO_FEAT_CURV = 1, PO_FEAT_CURV_RATE = 2, PO_FEAT_KMAX = 3,
       PO_FEAT_CLR_MIN = 4, PO_FEAT_PROX = 5, PO_FEAT_GOAL = 6, PO_FEAT_DEV_PREV = 7, PO_N_FEAT = 8 };
typedef struct po_select_params {
    double w[PO_N_FEAT];      /* cost weights, finite */
    double d_safe;            /* proximity penalty starts below this clearance */
    double min_clearance;     /* feasible iff CLR_MIN >= min_clearance */
    double max_kmax;          /* feasible iff KMAX <= max_kmax */
    double max_goal_dist;     /* feasible iff GOAL <= max_goal_dist */
} po_select_params;
void po_default_select_params(po_select_params *p);
typedef struct po_select_in {
    int B, N;                     /* candidates, rows per candidate (stride) */
    const double *states;         /* [B][N][5] x, y, heading, k, s : po_plan_out.states / po_batch_out states */
    const int    *n_states;       /* optional [B] (NULL: N) */
    const int    *ok;             /* optional [B] (NULL: all 1) : po_plan_out.ok / po_postcheck ok */
    const double *goal;           /* optional [B][goal_stride], x, y first : po_plan_in.goal */
    int goal_stride;
    int G;                        /* groups */
    const int    *group_start;    /* [G+1]: group g = candidates [group_start[g], group_start[g+1]) */
    int Np;                       /* rows per previous path (stride); 0: none */
    const double *prev_states;    /* optional [G][Np][5]: last cycle's sel_states */
    const int    *prev_n;         /* optional [G] (NULL: Np) : last cycle's sel_n */
} po_select_in;
typedef struct po_select_out {
    double *feat;        /* optional [B][PO_N_FEAT] */
    double *cost;        /* optional [B]; +inf = infeasible */
    int    *best;        /* [G]: candidate index, -1 = no feasible candidate */
    double *best_cost;   /* optional [G] */
    int    *n_feasible;  /* optional [G] */
    double *sel_states;  /* optional [G][N][5]: the winners' rows, zero beyond sel_n */
    int    *sel_n;       /* [G] when sel_states is given */
} po_select_out;
int po_select_batch(po_handle h, const po_select_params *p, const po_select_in *in, const po_select_out *out);         /* host pointers, synchronous */
int po_select_batch_device(po_handle h, const po_select_params *p, const po_select_in *in, const po_select_out *out);  /* device pointers, on the stream, no synchronisation */

/* ---- speed profile: v, a and t for every state of B planned paths (csrc/po_speed.hip) ----
 * Every path the chain returns has State.v = State.a = 0, as in the reference.  This stage gives a path its time parameterisation on the device — the classic
 * forward / backward pass over squared speed — and with it the two arrays po_limits_batch* (updateLimits) consumes: out->v and out->a have its [B][N] layout, so
 * select -> speed -> limits -> a KPC solve needs no host round trip.  `states` is the [B][N][5] layout of po_plan_out.states, po_batch_out states and
 * po_select_out.sel_states.  The reference has no such stage.
 *
 * Definition (the bar is BIT equality).  Every operation is one rounded IEEE double operation in the order written, nothing contracted; sqrt and / are the
 * correctly rounded ones; a comparison with a NaN is false; min(a, b) = b < a ? b : a; max(a, b) = b > a ? b : a.  g = 9.8; A = mu * g (mu of the handle's
 * po_params; one multiply, as updateLimits forms it); R = po_params.max_curvature_rate.  n = n_states[b] clamped into [0, N] (N when NULL); row i = (x_i, y_i, z_i, k_i, s_i).
 *   Not profiled: status = 0 and the v, a, t rows and total_time are all zero when ok[b] == 0, or n < 2, or v0[b] is not a finite value >= 0, or any k or s of
 *       rows < n is non-finite, or (use_map) any x, y or heading of rows < n is non-finite.
 *   Otherwise, with ds_i = s_{i+1} - s_i and d_i = ds_i > 0 ? ds_i : 0:
 *   1. Caps, per state i < n, in squared speed.  W_i = v_max * v_max, then in this order:
 *       lateral:    ak = |k_i|;  if ak > 0: W_i = min(W_i, a_lat_max / ak).
 *       rate:       r_j = ds_j > 0 ? |k_{j+1} - k_j| / ds_j : 0 for interval j;  rr = 0;  if i > 0: rr = max(rr, r_{i-1});  if i < n - 1: rr = max(rr, r_i);
 *                   if rr > 0: q = R / rr, W_i = min(W_i, q * q).
 *       per state:  if v_limit is given and l = v_limit[b][i] >= 0 (a negative or NaN entry is no limit): W_i = min(W_i, l * l).
 *       clearance:  if use_map: c_i = the per-state clearance of po_select_batch's definition (six circles, the layer of instance b);  cc = c_i > 0 ? c_i : 0,
 *                   vc = clear_v0 + clear_gain * cc, W_i = min(W_i, vc * vc).
 *   2. Forward pass.  w_0 = min(W_0, v0 * v0).  For i = 0 .. n - 2:  lat = w_i * |k_i|;  rem = A * A - lat * lat;  rem = rem > 0 ? rem : 0;
 *       ax = min(sqrt(rem), a_max);  w_{i+1} = min(W_{i+1}, w_i + (2 * ax) * d_i).
 *   3. Backward pass.  If v_end is given and e = v_end[b] is a finite value >= 0: w_{n-1} = min(w_{n-1}, e * e).  For i = n - 2 .. 0:
 *       lat = w_{i+1} * |k_{i+1}|;  rem as above;  bx = min(sqrt(rem), b_max);  w_i = min(w_i, w_{i+1} + (2 * bx) * d_i).
 *   4. Outputs.  v_i = sqrt(w_i).  For i < n - 1: a_i = ds_i > 0 ? (w_{i+1} - w_i) / (2 * ds_i) : 0, then a_i = max(-A, min(a_i, A));  a_{n-1} = 0.
 *       t_0 = 0;  vs = v_i + v_{i+1};  t_{i+1} = t_i + (vs > 0 ? (2 * d_i) / vs : 0).  total_time = t_{n-1}.  Rows >= n are zero.
 *       status = 2 when the final w_0 < v0 * v0 (the vehicle enters faster than the caps and the braking limits allow), else 1.
 *   The clamp on a: rounding otherwise leaves |a| an ulp above A on friction-limited intervals, and updateLimits' sqrt(A^2 - a^2) would be NaN; with the clamp
 *       a * a <= A * A holds in rounded arithmetic.
 *   Known property, stated and not fixed: an interval's friction bound is evaluated at the state the pass comes from, so a_i^2 + (w_i k_i)^2 can exceed A^2 on
 *       braking intervals.  No claim is made about it.
 * Return codes.  PO_ERR_INVALID: a NULL handle, struct or required pointer (B > 0: states, v0, v, a, status); a negative B or N; a parameter outside the ranges
 *   given at po_speed_params (all seven are checked whatever use_map says), or NaN; use_map with no map or with an assignment shorter than B (the rule of
 *   po_bounds_batch*).  B = 0: PO_OK, nothing is launched and nothing is written — decided after the argument and parameter checks and BEFORE the map rule.
 *   use_map = 0 reads no map and works on a handle without one.
 * `p` is a host pointer in both entries.  out->v doubles as the buffer between the two kernels (W, then w, then v): no scratch is allocated.  Deterministic: no
 * atomics, and a path's results depend neither on the batch size nor on its position in the batch.
 * po_default_speed_params: {15, 3, 2, 3, 1, 2, 0} — a starting point nobody has tuned. */
typedef struct po_speed_params {
    double v_max;       /* > 0, finite */
    double a_lat_max;   /* 0 < a_lat_max <= mu * 9.8 */
    double a_max;       /* > 0: forward acceleration cap */
    double b_max;       /* > 0: braking cap */
    double clear_v0;    /* >= 0: speed allowed at clearance <= 0 (use_map only) */
    double clear_gain;  /* >= 0: speed per metre of clearance, 1/s (use_map only) */
    int    use_map;     /* 0: no map is read and none is needed */
} po_speed_params;
void po_default_speed_params(po_speed_params *p);
typedef struct po_speed_in {
    int B, N;                /* paths, rows per path (stride) */
    const double *states;    /* [B][N][5] x, y, heading, k, s */
    const int    *n_states;  /* optional [B] (NULL: N) */
    const int    *ok;        /* optional [B] (NULL: all 1) */
    const double *v0;        /* [B] start speed */
    const double *v_end;     /* optional [B] end speed (NULL: free) */
    const double *v_limit;   /* optional [B][N]: per-state speed limit, a negative or NaN entry = none */
} po_speed_in;
typedef struct po_speed_out {
    double *v, *a;           /* [B][N] — the layout po_limits_batch* reads */
    double *t;               /* optional [B][N] */
    double *total_time;      /* optional [B] */
    int    *status;          /* [B]: 0 not profiled, 1 profiled, 2 profiled and entering too fast */
} po_speed_out;
int po_speed_batch(po_handle h, const po_speed_params *p, const po_speed_in *in, const po_speed_out *out);         /* host pointers, synchronous */
int po_speed_batch_device(po_handle h, const po_speed_params *p, const po_speed_in *in, const po_speed_out *out);  /* device pointers, on the stream, no synchronisation */

/* ---- moving obstacles: B timed paths against predicted agents (csrc/po_dynamic.hip) ----
 * Every obstacle of the stages above is static, and nothing reads the t po_speed_batch* writes.  This stage takes B timed paths (states and po_speed_out.t) and,
 * per instance, a SET of agents that move along piecewise-linear predicted trajectories; it computes the continuous-time closest approach between the six
 * footprint circles and every agent of the set, reports the first conflict and writes the v_limit rows that make po_speed_batch* stop short of it.  out->v_limit
 * has the layout of po_speed_in.v_limit and out->ok_out that of po_select_in.ok, so speed -> dynamic -> speed (yield) and speed -> dynamic -> select (prefer the
 * conflict-free candidates) stay on one stream.  The stage reads no map and works on a handle without one.  The reference has no such stage.
 *
 * Definition (the bar is BIT equality).  Every operation is one rounded IEEE double operation in the order written, nothing contracted; sqrt and / are the
 * correctly rounded ones; a comparison with a NaN is false; min(a, b) = b < a ? b : a; max(a, b) = b > a ? b : a.  n = n_states[b] clamped into [0, N] (N when
 * NULL); row i = (x_i, y_i, z_i, k_i, s_i); t_i = t[b][i].  L(i) = v_limit_in[b][i], -1 when v_limit_in is NULL.
 *   Not checked: status = 0, ok_out = 0, gap_min = DBL_MAX, first_state = first_agent = stop_state = -1, first_time = 0, every entry of the gap row DBL_MAX and
 *       v_limit[i] = L(i) for every i < N, when ok[b] == 0, or n < 2, or any x, y, z or t of rows < n is non-finite.
 *   Circle centres, per state i < n and circle q = 0 .. 5 (po_select_batch's, the bounding circle is not used):  cz = pcos(z_i), sz = psin(z_i);
 *       gx_iq = (cx_q * cz - cy_q * sz) + x_i,  gy_iq = (cx_q * sz + cy_q * cz) + y_i.
 *   The agents of path b: k = set_of[b] clamped into [0, S - 1] (0 when NULL); lo = first[k], hi = first[k + 1], each clamped into [0, n_agents]; agents lo .. hi - 1
 *       of agents[], ascending (none when hi <= lo).  Agent a has np = n_pts points (T_j, X_j, Y_j), j < np, and radius R.  It covers nothing when np < 1, np > 8,
 *       !(R >= 0), or any T_j, X_j, Y_j with j < np is non-finite.  Otherwise its pieces are, in this order:
 *       before (flags & PO_AGENT_HOLD_BEFORE):  stationary at point 0 for all times <= T_0;
 *       segment j = 0 .. np - 2:  D = T_{j+1} - T_j, skipped unless D > 0; linear in time on [T_j, T_{j+1}];
 *       after (flags & PO_AGENT_HOLD_AFTER):  stationary at point np - 1 for all times >= T_{np-1}.
 *   Interval i < n - 1 is CHECKED when dt = t_{i+1} - t_i > 0.  An interval of zero duration is skipped — so the states that share their time with a predecessor
 *       are never reached, which is what makes a yielded profile (v = 0 from the stop state on) end at its stop — and so is one of negative duration.  What arrives
 *       at a vehicle after it has stopped for good is outside this stage.
 *   Per checked interval i and piece, the window [ta, tb] and the agent's positions (ax_a, ay_a) at ta and (ax_b, ay_b) at tb:
 *       before:   ta = t_i;  tb = min(t_{i+1}, T_0);  both positions (X_0, Y_0).
 *       segment:  ta = max(t_i, T_j);  tb = min(t_{i+1}, T_{j+1});  wa = (ta - T_j) / D, wb = (tb - T_j) / D;
 *                 ax_a = X_j + wa * (X_{j+1} - X_j), ay_a = Y_j + wa * (Y_{j+1} - Y_j), and the same with wb for (ax_b, ay_b).
 *       after:    ta = max(t_i, T_{np-1});  tb = t_{i+1};  both positions (X_{np-1}, Y_{np-1}).
 *       The piece is skipped unless ta <= tb.  ua = (ta - t_i) / dt, ub = (tb - t_i) / dt.  Then for q = 0 .. 5:
 *       ex_a = gx_iq + ua * (gx_{i+1,q} - gx_iq), ey_a = gy_iq + ua * (gy_{i+1,q} - gy_iq), and the same with ub for (ex_b, ey_b);
 *       rax = ex_a - ax_a, ray = ey_a - ay_a, rbx = ex_b - ax_b, rby = ey_b - ay_b;   dx = rbx - rax, dy = rby - ray, px = -rax, py = -ray;
 *       L2 = dx * dx + dy * dy, dot = px * dx + py * dy;   u = L2 > 0 ? dot / L2 : 0, then u = u < 0 ? 0 : u, then u = u > 1 ? 1 : u   (the form of select's e_i);
 *       qx = px - u * dx, qy = py - u * dy;   dist = sqrt(qx * qx + qy * qy);   gap = (dist - cr_q) - R.
 *   Reductions.  gap_i = DBL_MAX and arg_i = -1; then for every evaluation on interval i, agents ascending, pieces in the order above, q ascending:
 *       if gap < gap_i: gap_i = gap, arg_i = a (the index into agents[]) — so arg_i is the agent with the smallest gap, the smallest index among equals.  gap_i stays
 *       DBL_MAX for an interval that is not checked and for every i >= n - 1.  gap_min = the minimum of the gap_i (never a NaN and never -0: any order gives the
 *       same bits).  f = the smallest i with gap_i < margin.  None: the path is FREE — status = 1, ok_out = 1, first_state = first_agent = stop_state = -1,
 *       first_time = 0, v_limit[i] = L(i) for every i < N.  Otherwise first_state = f, first_agent = arg_f, first_time = t_f, ok_out = 0, and
 *   the stop rule:  s_stop = s_f - stop_distance;  stop_state = j = the largest i <= f with s_i <= s_stop, 0 when there is none;  status = 3 when !(s_0 <= s_stop)
 *       (the conflict is nearer than stop_distance), else 2;  v_limit[i] = 0 for j <= i < n and L(i) for every other i < N.
 * Sets.  agents->first[S + 1]: set k = agents [first[k], first[k+1]).  Agents come in sets so that one call serves many vehicles or perception hypotheses, as the
 *   map stack does; set_of is an argument and not the handle's map assignment because the stage reads no map — a caller who wants "the agents of my layer"
 *   passes the same array to both.  Empty sets and n_agents = 0 are valid: every checked path is free.
 * Return codes, both entries.  PO_ERR_INVALID: a NULL handle, struct or required pointer (B > 0: states, t, status, agents; inside agents: first, and agents when
 *   n_agents > 0); a negative B, N, S or n_agents; S = 0 with B > 0; a margin that is not finite; a stop_distance that is negative or not finite.  The HOST entry
 *   reads the lists and refuses, before it touches the handle: first[0] != 0, a decreasing first, first[S] > n_agents; a set_of[b] outside [0, S); an agent with
 *   n_pts outside 1 .. 8, a negative or non-finite radius, a non-finite t, x or y among its points, t that is not strictly increasing, or unknown flag bits.
 *   The DEVICE entry cannot look at the lists: its kernel reads set_of, first and n_pts as the definition says (clamped, or covering nothing), so a bad list
 *   checks wrongly and never reads outside the buffers.  B = 0: PO_OK, nothing is launched and nothing is written — decided after the argument checks.
 * `p`, `in->agents` (the struct) are host pointers in both entries; the arrays inside are device pointers for the device entry.  Deterministic: no atomics, no
 * scratch, and a path's results depend neither on the batch size nor on its position in the batch.
 * po_default_dynamic_params: {0.3, 5.0} — a starting point nobody has tuned. */
#define PO_AGENT_MAX_PTS 8
#define PO_AGENT_HOLD_BEFORE 1   /* present at (x[0], y[0]) for all times before t[0] */
#define PO_AGENT_HOLD_AFTER  2   /* present at the last point for all times after the last t */
typedef struct po_agent {        /* 208 bytes */
    int n_pts, flags;            /* 1 .. PO_AGENT_MAX_PTS points; PO_AGENT_HOLD_* */
    double radius;               /* >= 0 */
    double t[PO_AGENT_MAX_PTS], x[PO_AGENT_MAX_PTS], y[PO_AGENT_MAX_PTS];  /* t strictly increasing */
} po_agent;
typedef struct po_agent_lists {
    const po_agent *agents;      /* [n_agents] */
    const int *first;            /* [S+1]: set k = agents [first[k], first[k+1]) */
    int n_agents, S;
} po_agent_lists;
typedef struct po_dynamic_params {
    double margin;               /* conflict <=> gap < margin; finite */
    double stop_distance;        /* >= 0, finite: stop this far (arc length) before the conflict */
} po_dynamic_params;
void po_default_dynamic_params(po_dynamic_params *p);
typedef struct po_dynamic_in {
    int B, N;                    /* paths, rows per path (stride) */
    const double *states;        /* [B][N][5] x, y, heading, k, s */
    const int    *n_states;      /* optional [B] (NULL: N) */
    const int    *ok;            /* optional [B] (NULL: all 1) */
    const double *t;             /* [B][N]: po_speed_out.t */
    const int    *set_of;        /* optional [B] (NULL: set 0): instance b meets agents [first[set_of[b]], first[set_of[b]+1]) */
    const po_agent_lists *agents;
    const double *v_limit_in;    /* optional [B][N], merged into v_limit */
} po_dynamic_in;
typedef struct po_dynamic_out {
    int    *status;              /* [B] 0 not checked, 1 free, 2 conflict, 3 conflict nearer than stop_distance */
    int    *ok_out;              /* optional [B]: status == 1, the layout of po_select_in.ok */
    double *gap_min;             /* optional [B] */
    int    *first_state, *first_agent, *stop_state; /* optional [B]; -1 when free */
    double *first_time;          /* optional [B] */
    double *gap;                 /* optional [B][N]: per interval, min over agents */
    double *v_limit;             /* optional [B][N]: the layout of po_speed_in.v_limit */
} po_dynamic_out;
int po_dynamic_batch(po_handle h, const po_dynamic_params *p, const po_dynamic_in *in, const po_dynamic_out *out);         /* host pointers, synchronous */
int po_dynamic_batch_device(po_handle h, const po_dynamic_params *p, const po_dynamic_in *in, const po_dynamic_out *out);  /* device pointers, on the stream, no synchronisation */

/* ---- station-time speed planning: pass or yield around predicted agents (csrc/po_stplan.hip) ----
 * po_dynamic_batch* knows one remedy: stop short of the first conflict.  This stage decides between easing off, yielding and passing ahead.  Per path it lays
 * stations along the path, marks every (time window, station) cell an agent of the path's set blocks, and searches the station-time graph for the cheapest
 * speed plan through the free cells.  out->v_limit has the layout of po_speed_in.v_limit, so stplan -> speed -> dynamic stays on one stream.  The stage reads no
 * map and works on a handle without one.  The reference has no such stage.
 *
 * Definition (the bar is BIT equality).  The conventions are po_dynamic_batch's: every operation is one rounded IEEE double operation in the order written,
 * nothing contracted; sqrt and / are the correctly rounded ones; a comparison with a NaN is false; min(a, b) = b < a ? b : a; max(a, b) = b > a ? b : a.
 * n = n_states[b] clamped into [0, N] (N when NULL); row i = (x_i, y_i, z_i, k_i, s_i).  L(i) = v_limit_in[b][i], -1 when v_limit_in is NULL.  Integer divisions
 * truncate.  K, stride, U, dt, margin, a_max, b_max, v_max, w_acc, w_slow are the fields of po_stplan_params.
 *   Not planned: status = 0, ok_out = 0, n_layers = 0, cost = DBL_MAX, every entry of the station row and of the cells row -1 and v_limit[i] = L(i) for every
 *       i < N, when ok[b] == 0, or n < 2, or v0[b] is not a finite value >= 0, or any x, y, z or s of rows < n is non-finite, or M < 2.
 *   Stations.  M = min((n - 1) / stride + 1, PO_ST_MAX_STATIONS).  Station m < M is state m * stride; S_m = its s.  Vc_m = v_max; when v_cap is given and
 *       e = v_cap[b][m * stride] satisfies e >= 0: Vc_m = min(Vc_m, e).  The circle centres gx_mq, gy_mq, q = 0 .. 5, are po_dynamic_batch's at that state.
 *   Blocked cells.  One cell (k, m) for every k < K, m < M: the window [tk, tk1], tk = (double)k * dt, tk1 = (double)(k + 1) * dt, with the ego standing still
 *       at station m.  The agents of path b are po_dynamic_batch's (set_of clamped, first clamped, agents that cover nothing by the same rule), ascending; each
 *       agent's pieces come in po_dynamic_batch's order with its window formulas, t_i := tk and t_{i+1} := tk1; a piece is skipped unless ta <= tb.  For
 *       q = 0 .. 5:  rax = gx_mq - ax_a, ray = gy_mq - ay_a, rbx = gx_mq - ax_b, rby = gy_mq - ay_b;  then po_dynamic_batch's dx, dy, px, py, L2, dot, u (clamped),
 *       qx, qy, dist and gap = (dist - cr_q) - R.  cell(k, m) = the smallest agent index (into agents[]) with some gap < margin, -1 when there is none.
 *       Known and not fixed: an edge of the search counts the vehicle as present at every station it sweeps, for the whole window — conservative; between two
 *       stations only the margin covers the vehicle.
 *   Step table, for 0 <= u <= min(U, j), j < M:  v(j, u) = (S_j - S_{j-u}) / dt;  c(j, u): c = Vc_{j-u}, then c = min(c, Vc_m) for m = j - u + 1 .. j, ascending.
 *       (j, u) is DRIVABLE iff u == 0, or v(j, u) > 0 and v(j, u) <= c(j, u).  It is CLEAR in window k iff no cell (k, m), m = j - u .. j, is blocked.
 *   Search.  Every state holds DBL_MAX until a feasible edge reaches it; a state is REACHABLE iff its value is < DBL_MAX.  Layer 0 has one state: station 0 with
 *       the previous speed v0 and the value 0.  For k = 1 .. K, state (j, u) of layer k looks at its predecessors (j - u, u') of layer k - 1, u' = 0 .. min(U, j - u)
 *       ascending (for k = 1: the one state of layer 0, which needs j - u == 0; its back pointer is 0), and takes  cand = C_{k-1}(j - u, u') + e  when the edge is
 *       feasible and cand < the value held (strict: the smallest u' among equals); the back pointer is the winning u'.
 *       vp = v0 for k = 1, else v(j - u, u');  acc = (v(j, u) - vp) / dt;  dv = c(j, u) - v(j, u);  e = (w_acc * acc) * acc + (w_slow * dv) * dv.
 *       The edge is feasible iff the predecessor is reachable and has not ARRIVED (j - u != M - 1), (j, u) is drivable and clear in window k - 1,
 *       acc <= a_max and acc >= -b_max, and, for k > 1, u' == 0 implies u == 0: a speed profile over arc length cannot express stop, wait, go — po_dynamic_batch's
 *       own statement about stops — so a vehicle that has stopped stays stopped to the horizon.  (po_stgo_batch*, below, is this search without that clause:
 *       its plans stop, wait and go, and leave sampled in time, not as a v_limit row.)
 *   Choice.  The candidates are the states (k, M - 1, u), k = 1 .. K (arrived), and every state of layer K.  Scan k ascending, then j, then u, and take a
 *       candidate when its value < the best so far (starting at DBL_MAX).  None: status = 3 and the outputs of "not planned" except that the cells row is the map.
 *       Otherwise n_layers = the chosen k, cost = its value, station[0 .. n_layers] = the stations along the back pointers (station[0] = 0) and -1 behind them,
 *       u_k = station[k] - station[k-1];  status = 1 when no cell of the map is blocked, else 2;  ok_out = 1.
 *   v_limit.  i >= n: L(i).  i < n: m = i / stride.  m >= station[n_layers]: 0 when u_{n_layers} == 0, else L(i).  Otherwise, with the one k such that
 *       station[k] <= m < station[k+1]:  V = v(station[k+1], u_{k+1});  the value is L(i) >= 0 ? min(L(i), V) : V.
 *   cells [B][K][PO_ST_MAX_STATIONS]: cell(k, m) for m < M, -1 in the columns >= M — there so that the geometry half and the search half can be checked apart.
 * Return codes, both entries.  PO_ERR_INVALID: a NULL handle, struct or required pointer (B > 0: states, v0, status, agents; inside agents: first, and agents
 *   when n_agents > 0); a negative B, N, S or n_agents; S = 0 with B > 0; dt, a_max, b_max or v_max not finite or not > 0; K outside 1 .. PO_ST_MAX_LAYERS;
 *   stride < 1; U outside 1 .. PO_ST_MAX_STEP; margin not finite; w_acc or w_slow negative or not finite.  The HOST entry refuses the lists po_dynamic_batch
 *   refuses; the DEVICE entry reads them clamped, as the definition says, and never reads outside the buffers.  B = 0: PO_OK after those checks, nothing launched.
 * `p`, `in->agents` (the struct) are host pointers in both entries; the arrays inside are device pointers for the device entry.  Deterministic: no atomics, no
 * scratch, and a path's results depend neither on the batch size nor on its position in the batch.
 * po_default_stplan_params: {1.0, 8, 3, 20, 0.5, 2, 3, 15, 1, 1} — a starting point nobody has tuned. */
#define PO_ST_MAX_LAYERS 16
#define PO_ST_MAX_STEP 31
#define PO_ST_MAX_STATIONS 128
typedef struct po_stplan_params {
    double dt;                   /* > 0, finite: time step */
    int K;                       /* 1 .. PO_ST_MAX_LAYERS steps; the horizon is K * dt */
    int stride;                  /* >= 1: path states per station */
    int U;                       /* 1 .. PO_ST_MAX_STEP: most stations advanced in one step */
    double margin;               /* finite: a cell is blocked <=> gap < margin */
    double a_max, b_max;         /* > 0, finite: acceleration and braking limits */
    double v_max;                /* > 0, finite: speed cap */
    double w_acc, w_slow;        /* >= 0, finite: cost weights */
} po_stplan_params;
void po_default_stplan_params(po_stplan_params *p);
typedef struct po_stplan_in {
    int B, N;                    /* paths, rows per path (stride of the arrays) */
    const double *states;        /* [B][N][5] x, y, heading, k, s */
    const int    *n_states;      /* optional [B] (NULL: N) */
    const int    *ok;            /* optional [B] (NULL: all 1) */
    const double *v0;            /* [B] */
    const double *v_cap;         /* optional [B][N]: a per-state speed cap (po_speed_out.v of a profile without agents); negative or NaN: none */
    const int    *set_of;        /* optional [B] (NULL: set 0) */
    const po_agent_lists *agents;
    const double *v_limit_in;    /* optional [B][N], merged into v_limit */
} po_stplan_in;
typedef struct po_stplan_out {
    int    *status;              /* [B] 0 not planned, 1 planned and no cell blocked, 2 planned around blocked cells, 3 no plan */
    int    *ok_out;              /* optional [B]: status 1 or 2 */
    int    *n_layers;            /* optional [B] */
    double *cost;                /* optional [B] */
    int    *station;             /* optional [B][PO_ST_MAX_LAYERS + 1] */
    int    *cells;               /* optional [B][K][PO_ST_MAX_STATIONS] */
    double *v_limit;             /* optional [B][N]: the layout of po_speed_in.v_limit */
} po_stplan_out;
int po_stplan_batch(po_handle h, const po_stplan_params *p, const po_stplan_in *in, const po_stplan_out *out);         /* host pointers, synchronous */
int po_stplan_batch_device(po_handle h, const po_stplan_params *p, const po_stplan_in *in, const po_stplan_out *out);  /* device pointers, on the stream, no synchronisation */

/* ---- corridor nudge: carve predicted agents out of the corridor bounds, pass left or right (csrc/po_nudge.hip) ----
 * po_dynamic_batch* and po_stplan_batch* answer an agent with speed.  This stage answers with steering: per path it takes the corridor po_bounds_batch* wrote
 * (lb, ub per state and covering circle), finds for every agent of the path's set the lateral interval it occupies at the states the vehicle reaches while the
 * agent is there, decides per agent whether the vehicle passes LEFT or RIGHT of it, and moves the lower or the upper bound of the touched pairs to the
 * interval's edge.  out->bounds has the layout of po_batch_in.bounds, so bounds -> nudge -> QP -> speed -> dynamic / stplan stays on one stream.  An agent that
 * leaves no side to pass on is reported (status 3) and the caller hands it to the speed stages.  The stage reads no map and works on a handle without one.  The
 * reference has no such stage.
 *
 * Definition (the bar is BIT equality).  The conventions are po_dynamic_batch's: every operation is one rounded IEEE double operation in the order written,
 * nothing contracted; sqrt and / are the correctly rounded ones; a comparison with a NaN is false; min(a, b) = b < a ? b : a; max(a, b) = b > a ? b : a.
 * margin, t_before, t_after, min_width, skip_states are the fields of po_nudge_params.  n = n_points[b] clamped into [0, N] (N when NULL); x_i, y_i, z_i =
 * ref_x, ref_y, ref_z[b][i]; t_i = t[b][i]; lb_ij = bounds[b][i][j][0], ub_ij = bounds[b][i][j][1], j = 0 .. 3.  rad = sqrt((car_length / 8) * (car_length / 8) +
 * (car_width / 2) * (car_width / 2)) + safety_margin of the handle's parameters (the radius po_bounds_batch* derives); d_j = po_params.d[j].
 *   Not processed: status = 0, ok_out = 0, out->bounds equal to in->bounds in all N rows, side[b][e] = 0 for every e < W, first_blocked_state =
 *       first_blocked_agent = -1, width_min = DBL_MAX, when ok[b] == 0, or n < 1, or any x, y, z, t or bound of rows < n is non-finite.
 *   Working corridor: Wl_ij = lb_ij, Wu_ij = ub_ij.
 *   Frame of pair (i, j), i < n:  cz = pcos(z_i), sz = psin(z_i);  cx = x_i + d_j * cz, cy = y_i + d_j * sz.  A world point (X, Y) has, with dx = X - cx and
 *       dy = Y - cy, the longitudinal coordinate u = dx * cz + dy * sz and the lateral coordinate l = (-dx) * sz + dy * cz, left positive (bounds_kernel's off).
 *   Window of state i:  w0_i = t_i - t_before,  w1_i = t_i + t_after.
 *   The agents of path b are po_dynamic_batch's: k = set_of[b] clamped into [0, S - 1] (0 when NULL), first[k] and first[k + 1] clamped into [0, n_agents],
 *       ascending; e = a - first[k] (clamped) is the agent's index within the set.  An agent that covers nothing by po_dynamic_batch's rule has side 0 and
 *       changes nothing.  Otherwise rho = (rad + R) + margin.
 *   Hull of one agent on one pair: lo = DBL_MAX, hi = -DBL_MAX.  The agent's pieces come in po_dynamic_batch's order with its window formulas, t_i := w0_i and
 *       t_{i+1} := w1_i (the substitution po_stplan_batch makes): the same ta, tb, wa, wb and positions (ax_a, ay_a), (ax_b, ay_b); a piece is skipped unless
 *       ta <= tb.  (ua, la) and (ub, lb) are the two positions in the pair's frame.  Every candidate c below is folded in as lo = min(lo, c), hi = max(hi, c),
 *       in this order:
 *       end a:  q = rho * rho - ua * ua;  if q >= 0:  w = sqrt(q);  candidates la - w, then la + w.
 *       end b:  the same with (ub, lb).
 *       sides:  du = ub - ua, dl = lb - la, L2 = du * du + dl * dl;  only if L2 > 0 and du != 0:  len = sqrt(L2), ox = (rho * dl) / len, oy = (rho * du) / len;
 *               tp = (ox - ua) / du;  if 0 <= tp and tp <= 1: candidate (la + oy) + tp * dl;   tm = (0 - (ox + ua)) / du;  if 0 <= tm and tm <= 1: candidate
 *               (la - oy) + tm * dl.
 *       Per piece this is exactly the lateral interval in which a circle centre of this pair comes within rho of the agent's swept segment; over several
 *       pieces it is their hull, which is conservative (an agent that turns around a corner also takes the room inside the corner).
 *   Pair (i, j) is TOUCHED by the agent iff i >= skip_states and lo <= hi and hi > Wl_ij and lo < Wu_ij.
 *   Decision per agent, over its touched pairs: rl = the minimum of Wu_ij - hi, rr = the minimum of lo - Wl_ij (minima of doubles that are never NaN: see the
 *       decision below; any order gives the same comparisons), f = the smallest touched i.  Then, in this order:
 *       no touched pair: side = 0.  Left is passable iff rl >= min_width, right iff rr >= min_width.  sp = side_prev[b][e] when side_prev is given and e < W,
 *       else 0.  sp == 1 and left passable: side = +1.  Else sp == -1 and right passable: side = -1.  Else both passable: side = +1 if rl >= rr, else -1.
 *       Else one side passable: that side.  Else side = 2: the corridor stays as it was, and if this is the first blocking agent of the path,
 *       first_blocked_agent = a (the index into agents[]) and first_blocked_state = f.
 *       side +1 (the vehicle passes LEFT of the agent): Wl_ij = hi on the touched pairs.  side -1: Wu_ij = lo on the touched pairs.  The next agent sees the
 *       corridor this one left, so the order of the agents in a set matters.
 *       Decided while building: a touched pair has a finite Wl and Wu and lo <= hi, but lo or hi may be infinite when the inputs are near DBL_MAX; rl and rr
 *       are then -inf, never NaN (a NaN candidate never enters lo or hi: its comparison is false), and the comparisons above hold as written.
 *   side[b][e] is written for e < W, 0 for e at or beyond the size of the set; agents with e >= W are processed and not recorded.
 *   Results.  out->bounds = the working corridor in rows < n and in->bounds in rows >= n.  width_min = the minimum over rows < n and j of Wu_ij - Wl_ij, folded
 *       with min from DBL_MAX; a term that is zero counts as +0.0 (decided while building: -0.0 - 0.0 is -0.0, and the minimum must not depend on the order
 *       of the fold).  status = 3 if any agent blocks, else 2 if some agent carved, else 1.  ok_out = status is 1 or 2.
 *       Carved rows may have lb > 0 or ub < 0 — the point of the stage; the QP entries take any bounds, and a corridor the QP cannot satisfy comes back from the
 *       solve as PO_STATUS_PRIMAL_INFEASIBLE.
 * Return codes, both entries.  PO_ERR_INVALID: a NULL handle, params, struct or required pointer (B > 0: ref_x, ref_y, ref_z, t, both bounds, status, agents;
 *   inside agents: first, and agents when n_agents > 0); out->bounds == in->bounds; a negative B, N, W, S, n_agents or skip_states; S = 0 with B > 0; side or
 *   side_prev given with W = 0; a margin that is not finite; a t_before, t_after or min_width that is negative or not finite.  The HOST entry refuses the lists
 *   po_dynamic_batch refuses; the DEVICE entry reads them clamped, as the definition says, and never reads outside the buffers.  A side_prev value other than
 *   +1 / -1 is no hint.  B = 0: PO_OK after those checks, nothing launched, nothing written.
 * `p`, `in->agents` (the struct) are host pointers in both entries; the arrays inside are device pointers for the device entry.  Deterministic: no atomics, no
 * scratch, and a path's results depend neither on the batch size nor on its position in the batch.
 * po_default_nudge_params: {0.3, 1.0, 1.0, 0.2, 0} — a starting point nobody has tuned. */
typedef struct po_nudge_params {
    double margin;               /* finite: extra clearance around an agent */
    double t_before, t_after;    /* >= 0, finite: the agent is considered over [t_i - t_before, t_i + t_after] */
    double min_width;            /* >= 0, finite: a side is passable iff every touched pair keeps this much room */
    int    skip_states;          /* >= 0: rows i < skip_states are never carved (a QP that pins its start) */
} po_nudge_params;
void po_default_nudge_params(po_nudge_params *p);
typedef struct po_nudge_in {
    int B, N, W;                 /* paths, rows per path (stride), stride of side / side_prev */
    const double *ref_x, *ref_y, *ref_z;   /* [B][N] reference states (po_batch_in's) */
    const int    *n_points;      /* optional [B] (NULL: N); po_bounds_batch's n_valid fits */
    const int    *ok;            /* optional [B] (NULL: all 1) */
    const double *t;             /* [B][N]: when the vehicle is expected at reference state i */
    const double *bounds;        /* [B][N][4][2] (lb, ub) per covering circle: po_bounds_batch's output */
    const int    *set_of;        /* optional [B], as po_dynamic_in */
    const po_agent_lists *agents;
    const int    *side_prev;     /* optional [B][W]: last cycle's side per agent of the set */
} po_nudge_in;
typedef struct po_nudge_out {
    int    *status;              /* [B] 0 not processed, 1 no agent touches the corridor, 2 carved, 3 at least one agent blocks */
    int    *ok_out;              /* optional [B]: status is 1 or 2 */
    double *bounds;              /* [B][N][4][2]: the layout of po_batch_in.bounds; must not alias in->bounds */
    int    *side;                /* optional [B][W]: per agent e of the set 0 untouched, +1 vehicle passes LEFT of it, -1 RIGHT, 2 blocks */
    int    *first_blocked_state, *first_blocked_agent;  /* optional [B]; -1 when none */
    double *width_min;           /* optional [B] */
} po_nudge_out;
int po_nudge_batch(po_handle h, const po_nudge_params *p, const po_nudge_in *in, const po_nudge_out *out);         /* host pointers, synchronous */
int po_nudge_batch_device(po_handle h, const po_nudge_params *p, const po_nudge_in *in, const po_nudge_out *out);  /* device pointers, on the stream, no synchronisation */

/* ---- timed trajectory: sample speed-profiled paths at uniform time steps, emit them as agents (csrc/po_trajectory.hip) ----
 * Everything the stages above produce is indexed by STATION: states[B][N][5] with v, a and t per state.  What leaves a planner is a trajectory sampled at
 * uniform TIME steps.  This stage inverts t(s) by po_speed_batch*'s own model (constant acceleration per interval, t_{i+1} = t_i + 2 d_i / (v_i + v_{i+1})),
 * so every consumer gets the same inversion; a stop, which a profile encodes as repeated times, comes out as a vehicle that stands at the stop state.  The same
 * samples can be written as po_agent records (up to PO_TRAJ_MAX_DISCS discs along the heading), which po_dynamic_batch_device, po_stplan_batch_device and
 * po_nudge_batch_device take as they are: vehicle A's plan is vehicle B's agent on the same stream.  out->states has the layout of every states array with
 * N := K, and with out->t it is a timed path po_dynamic_batch* reads.  The stage reads no map and works on a handle without one.  The reference has no such stage.
 *
 * Definition (the bar is BIT equality).  The conventions are po_dynamic_batch's: every operation is one rounded IEEE double operation in the order written,
 * nothing contracted; / is the correctly rounded one; a comparison with a NaN is false.  pcos and psin are po_pmath.h's.  t0, dt, K, D = n_discs, disc_offset,
 * disc_radius, P = agent_pts, agent_stride, agent_flags are the fields of po_trajectory_params.  n = n_states[b] clamped into [0, N] (N when NULL); row i =
 * (x_i, y_i, z_i, k_i, s_i); v_i = v[b][i], t_i = t[b][i].
 *   Not sampled: status = 0, every entry of the path's output rows (states, v, a, t) 0, every index -1, first_held = -1 and the path's D agent records all zero
 *       (n_pts = 0: they cover nothing by po_dynamic_batch's rule), when ok[b] == 0, or n < 1, or any x, y, z, k, s, v or t of rows < n is non-finite, or some
 *       v_i fails v_i >= 0, or t_{i+1} < t_i for some i < n - 1.
 *   End state E: the smallest i < n - 1 with v_i == 0, v_{i+1} == 0 and s_{i+1} - s_i > 0, and n - 1 when there is none: two states at rest with ground between
 *       them.  po_speed_batch's clock does not advance across such an interval and a vehicle does not cross it; on a yielded profile E is the stop state.
 *   Sample k < K:  T = t0 + (double)k * dt.  In this order:
 *       T >= t_E: HELD.  The sample is row E, with v = v_E, a = 0, index = E.
 *       Else T < t_0: the sample is row 0, with v = v_0, a = 0, index = 0.
 *       Else i = the largest index with t_i <= T.  Then i < E and t_{i+1} > T (t is non-decreasing, so the search method cannot change i), and
 *           Dt = t_{i+1} - t_i > 0;  tau = T - t_i;  acc = (v_{i+1} - v_i) / Dt;  sig = (v_i + (0.5 * acc) * tau) * tau;
 *           ds = s_{i+1} - s_i;  lam = ds > 0 ? sig / ds : 0, then lam = lam < 0 ? 0 : lam, then lam = lam > 1 ? 1 : lam;
 *           x = x_i + lam * (x_{i+1} - x_i), the same for y and k, and s = s_i + lam * ds;
 *           dz = z_{i+1} - z_i;  if dz > PI: dz = dz - TWO_PI, else if dz < -PI: dz = dz + TWO_PI  (the doubles 3.141592653589793 and 6.283185307179586);
 *           z = z_i + lam * dz, not wrapped again;
 *           vv = v_i + acc * tau, then v = vv > 0 ? vv : 0;  a = acc;  index = i.
 *       out->t[b][k] = T for every sample of a sampled path.
 *   first_held = the smallest k with T_k >= t_E, K when there is none (T_k is non-decreasing in k: a rounded product and a rounded sum are monotone).
 *   status = 1 when first_held == K: the whole horizon lies inside the path's time span.  Otherwise 2 when v_E == 0 (the vehicle stands there) and 3 when
 *       v_E > 0: the path ends AT SPEED before the horizon does, and the samples from first_held on repeat the end state — a vehicle that freezes where its plan
 *       ends, not one that drives on.  A caller that does not want that asks for a shorter horizon or a longer path.
 *   Agents, D > 0: the record at slot b * D + d, d < D, has n_pts = P, flags = agent_flags, radius = disc_radius[d]; point j < P is sample k = j * agent_stride
 *       with that sample's x, y, z and T:  t[j] = T,  x[j] = x + disc_offset[d] * pcos(z),  y[j] = y + disc_offset[d] * psin(z);  the points >= P are 0.  All
 *       208 bytes of every record are written.  covering discs: disc_offset = po_params.d[0 .. 3] and disc_radius = po_nudge_batch's rad cover the vehicle as the
 *       corridor stages see it (binding.covering_discs).
 *   Known and stated, not fixed: x and y are chords between states, not arcs.  Within an interval the motion is the constant-acceleration model the profile's t
 *       implies, not po_speed_batch's clamped a.  Where t0 + k * dt stops increasing in rounding, an agent's t is not strictly increasing; the HOST entry of
 *       po_dynamic_batch refuses such a list (the device entries skip the segment of zero duration).  Composing agent sets (first[]) from the records is the
 *       caller's job: a set is a contiguous range of slots.  (po_agentsets_batch*, below, composes them on the device: per ego path the records of the other
 *       vehicles and of a perception list that can matter to it, in the layout the consumers read.)
 *   Decided while building: disc_offset[d] and disc_radius[d] are checked for d < n_discs only, the entries behind are not read.  agent_pts, agent_stride and
 *       agent_flags are checked whatever n_discs is, so a struct that is refused with discs is refused without them.  (P - 1) * agent_stride is formed in 64 bits.
 *       "Aliasing" is an overlap of byte ranges: every output array given, over its full extent ([B][K][5], [B][K], [B], [B * D] records), against every input
 *       array given over its own; with B = 0 every extent is empty and nothing overlaps.  Two outputs that overlap each other are the caller's own affair.
 *       T = +inf (k * dt overflows) is held like any T >= t_E; T is never NaN because t0 and dt are finite.
 * Return codes, both entries.  PO_ERR_INVALID: a NULL handle, params or struct; a negative B or N; t0 not finite; dt not finite or not > 0; K < 1; n_discs outside
 *   0 .. PO_TRAJ_MAX_DISCS; a disc_offset that is not finite or a disc_radius that is negative or not finite (d < n_discs); agent_pts outside 1 .. PO_AGENT_MAX_PTS;
 *   agent_stride < 1; (agent_pts - 1) * agent_stride >= K; unknown agent_flags bits; with B > 0 a NULL in->states, in->v, in->t, out->status or out->states, and a
 *   NULL out->agents when n_discs > 0; an output that aliases an input.  B = 0: PO_OK after those checks, nothing launched, nothing written.
 * `p` is a host pointer in both entries.  Deterministic: no atomics, no scratch, and a path's results depend neither on the batch size nor on its position in
 * the batch.
 * po_default_trajectory_params: {0, 0.1, 50, 0, {0}, {0}, 8, 7, PO_AGENT_HOLD_AFTER} — 5 s at 10 Hz, no agents; eight points span the horizon (7 * 7 = 49 < 50).
 *   A starting point nobody has tuned. */
#define PO_TRAJ_MAX_DISCS 4
typedef struct po_trajectory_params {
    double t0, dt;               /* sample k is at T_k = t0 + (double)k * dt; t0 finite, dt > 0 and finite */
    int    K;                    /* >= 1 samples per path */
    int    n_discs;              /* D in 0 .. PO_TRAJ_MAX_DISCS: agent records written per path (0: none) */
    double disc_offset[PO_TRAJ_MAX_DISCS];  /* along the heading from the path point; finite */
    double disc_radius[PO_TRAJ_MAX_DISCS];  /* >= 0, finite */
    int    agent_pts;            /* P in 1 .. PO_AGENT_MAX_PTS */
    int    agent_stride;         /* >= 1: agent point j is sample j * agent_stride; (P - 1) * agent_stride < K */
    int    agent_flags;          /* PO_AGENT_HOLD_* bits only */
} po_trajectory_params;
void po_default_trajectory_params(po_trajectory_params *p);
typedef struct po_trajectory_in {
    int B, N;                    /* paths, rows per path (stride) */
    const double *states;        /* [B][N][5] x, y, heading, k, s */
    const int    *n_states;      /* optional [B] (NULL: N) */
    const int    *ok;            /* optional [B] (NULL: all 1) */
    const double *v, *t;         /* [B][N]: po_speed_out.v and po_speed_out.t */
} po_trajectory_in;
typedef struct po_trajectory_out {
    int    *status;              /* [B] 0 not sampled, 1 inside the path's time span, 2 held at rest, 3 held at speed (the path ends before the horizon) */
    double *states;              /* [B][K][5]: the states layout with N := K */
    double *v, *a, *t;           /* optional [B][K] */
    int    *index;               /* optional [B][K]: the state a sample is anchored at (i, E or 0); -1 when not sampled */
    int    *first_held;          /* optional [B]: K when no sample is held; -1 when not sampled */
    po_agent *agents;            /* [B * D] when D > 0: path b, disc d -> slot b * D + d */
} po_trajectory_out;
int po_trajectory_batch(po_handle h, const po_trajectory_params *p, const po_trajectory_in *in, const po_trajectory_out *out);         /* host pointers, synchronous */
int po_trajectory_batch_device(po_handle h, const po_trajectory_params *p, const po_trajectory_in *in, const po_trajectory_out *out);  /* device pointers, on the stream, no synchronisation */

/* ---- agent sets: per ego path, the agents that can matter to it (csrc/po_agentsets.hip) ----
 * The moving-obstacle stages read agents in SETS, contiguous ranges of one po_agent array, and po_trajectory_batch* writes a fleet's own plans as records at slot
 * b * D + d.  With three or more vehicles in a scene "everybody but me" is not a contiguous range, and a vehicle handed the whole range conflicts with its own
 * discs.  This stage composes the sets on the device: for each of B ego paths it copies, into one output array and in the po_agent_lists layout the three consumers
 * read, the records of a POOL (a set of the source lists: a world, a scene) that are not the ego's own and that come near the path in space and in time.  Two
 * sources: src[0], the fleet (po_trajectory_out.agents), where records have owners, and src[1], optional, a perception list nobody owns.  With it
 * speed -> trajectory -> agent sets -> dynamic / stplan / nudge stays on one stream for any number of vehicles.  The stage reads no map and works on a handle
 * without one.  The reference has no such stage.
 *
 * Definition (the bar is BIT equality with tests/agentsets_ref.py).  The conventions are po_dynamic_batch's: every operation is one rounded IEEE double operation
 * in the order written; a comparison with a NaN is false; min(a, b) = b < a ? b : a; max(a, b) = b > a ? b : a.  n = n_states[b] clamped into [0, N] (N when
 * NULL); row i = (x_i, y_i, ...); t_i = t[b][i].  reach, t_before, t_after, win_lo, win_hi, owner_div are the fields of po_agentsets_params.
 *   Not composed: status = 0, count = 0, an empty set (first[b + 1] == first[b]), when ok[b] == 0, or n < 1, or any x, y of rows < n is non-finite, or (with t
 *       given) any t of rows < n is non-finite.
 *   Path box and time span:  exl, exh, eyl, eyh = the minimum and maximum of x_i, y_i over rows < n.  With t: W0 = (min t_i) - t_before, W1 = (max t_i) + t_after
 *       (minimum and maximum, not first and last).  Without t: W0 = win_lo, W1 = win_hi.  These values only enter comparisons and are never written, so the order
 *       of the reductions and the sign of a zero cannot show.
 *   Candidates of ego b, in this order: the records of its pool of source 0, ascending, then those of its pool of source 1.  Pool of source s: k = pool_of[b]
 *       clamped into [0, S_s - 1] (0 when NULL); lo = first_s[k], hi = first_s[k + 1], each clamped into [0, n_agents_s]; records lo .. hi - 1 (none when hi <= lo).
 *       A NULL src[1], or one with S = 0 or n_agents = 0, contributes nothing.
 *   A candidate a (its index into the array of its source), with np = n_pts points (T_j, X_j, Y_j), radius R and flags, is KEPT iff all of these hold:
 *       it covers something by po_dynamic_batch's rule: 1 <= np <= 8, R >= 0, and every T_j, X_j, Y_j with j < np finite;
 *       source 0 only: its owner is not b.  The owner is owner[a] when owner is given, else a / owner_div when owner_div > 0, else there is none;
 *       time:  A0 <= W1 and A1 >= W0, where A0 = the minimum of T_j, j < np, or -inf with PO_AGENT_HOLD_BEFORE, and A1 = the maximum of T_j, or +inf with
 *           PO_AGENT_HOLD_AFTER (minimum and maximum because a device entry reads lists nobody validated; every piece the consumers walk lies in [A0, A1]);
 *       space: with rr = R + reach and axl, axh, ayl, ayh the minimum and maximum of X_j, Y_j, j < np:
 *           axl - rr <= exh,  axh + rr >= exl,  ayl - rr <= eyh,  ayh + rr >= eyl.
 *   Outputs.  count[b] = the number kept.  F_0 = 0, F_{b+1} = F_b + count[b] in 64 bits; first[b] = min(F_b, capacity) for b = 0 .. B.  The r-th kept candidate
 *       of ego b goes to slot p = F_b + r when p < capacity: all 208 bytes are copied as they are (the points at and behind n_pts too), and src_index[p] = a for
 *       source 0, src[0]->n_agents + a for source 1.  Slots at and behind first[B] are not written.  status[b] = 0 when not composed, otherwise 2 when
 *       F_b + count[b] > capacity, else 1.  total[0] = F_B.  set_of[b] = b.  A clipped set is a prefix of the full one: the caller sees it in status and total
 *       and calls again with room (capacity = 0 is the counting call).  {out->agents, out->first, n_agents = capacity, S = B} is a po_agent_lists, and with
 *       out->set_of as their set_of the consumers take it as it is.
 *   reach.  A po_dynamic_batch* with margin m cannot miss an agent when reach >= max_q (hypot(cx_q, cy_q) + cr_q) + m over the six footprint circles
 *       (binding.footprint_reach).  For po_nudge_batch* reach must also cover the corridor's width and d_j; for po_stplan_batch* the margin of that stage.
 *   Known and stated, not fixed: the box is that of the whole path, loose for long curved paths.  No nearest-first ordering and no cap per set: a clipped call
 *       clips the LAST sets.  Oriented-box agents are out of scope, as in the consumers.
 *   Decided while building: "overlap" is an overlap of byte ranges, out->agents over capacity records against each source array over its n_agents records.
 *       src[0]->n_agents + src[1]->n_agents must fit an int (src_index is one).  The HOST entry moves out->agents and out->src_index in both directions, so the
 *       slots that are not written keep the caller's bytes there too.
 * Return codes, both entries.  PO_ERR_INVALID: a NULL handle, params or struct; a negative B, N, capacity or owner_div; a reach, t_before or t_after that is
 *   negative or not finite; win_lo or win_hi not finite, or win_lo > win_hi; with B > 0 a NULL in->states, in->src[0], out->first, out->count or out->status, and a
 *   NULL out->agents when capacity > 0; src[0] refused as po_dynamic_batch refuses its lists (negative S or n_agents, S = 0, a NULL first, NULL agents with
 *   n_agents > 0), src[1] likewise unless it is NULL or has S = 0 or n_agents = 0; the two n_agents together beyond INT_MAX; out->agents overlapping a source array.  The HOST entry reads the lists and also
 *   refuses what po_dynamic_batch's host entry refuses, for both sources, with pool_of in the place of set_of.  The DEVICE entry reads everything clamped and never
 *   reads outside the buffers.  B = 0: PO_OK after those checks, nothing launched, nothing written.
 * `p`, `in->src[s]` (the structs) are host pointers in both entries; the arrays inside are device pointers for the device entry.  Deterministic: no atomics and no
 * scratch allocation (out->count and out->first carry the intermediates, so the entries only enqueue), and an ego's set, taken as contents and order, depends
 * neither on B nor on its position in the batch.
 * po_default_agentsets_params: {5.0, 0, 0, 0, 8, 0} — a starting point nobody has tuned. */
#define PO_SETS_SOURCES 2
typedef struct po_agentsets_params {
    double reach;               /* >= 0, finite: a record is kept when its box, grown by radius + reach, meets the path's box */
    double t_before, t_after;   /* >= 0, finite: the path's time span is widened by these (po_nudge_params' windows) */
    double win_lo, win_hi;      /* finite, win_lo <= win_hi: the time span when in->t is NULL (po_stplan: 0 and K * dt) */
    int    owner_div;           /* >= 0: without in->owner, record a of source 0 belongs to ego a / owner_div (po_trajectory's n_discs); 0: nobody owns it */
} po_agentsets_params;
void po_default_agentsets_params(po_agentsets_params *p);
typedef struct po_agentsets_in {
    int B, N;                   /* ego paths, rows per path (stride) */
    const double *states;       /* [B][N][5] x, y, heading, k, s */
    const int    *n_states;     /* optional [B] (NULL: N) */
    const int    *ok;           /* optional [B] (NULL: all 1) */
    const double *t;            /* optional [B][N]: po_speed_out.t */
    const po_agent_lists *src[PO_SETS_SOURCES]; /* src[0] required (the fleet: po_trajectory_out.agents), src[1] optional (perception); each in POOLS: first[S_s + 1] */
    const int    *pool_of;      /* optional [B] (NULL: pool 0): the pool of BOTH sources ego b draws from, clamped per source */
    const int    *owner;        /* optional [src[0]->n_agents]: the ego a record belongs to, or any value outside [0, B) for none */
} po_agentsets_in;
typedef struct po_agentsets_out {
    int        capacity;        /* records out->agents holds */
    po_agent  *agents;          /* [capacity] */
    int       *first;           /* [B + 1]: with agents and n_agents = capacity, S = B a po_agent_lists the consumers take */
    int       *count;           /* [B]: records kept for ego b, before clipping */
    int       *status;          /* [B] 0 not composed (empty set), 1 complete, 2 clipped by capacity */
    int       *set_of;          /* optional [B]: b, what the consumers take as set_of */
    int       *src_index;       /* optional [capacity]: where slot p came from: a (source 0) or src[0]->n_agents + a (source 1) */
    long long *total;           /* optional [1]: the sum of count */
} po_agentsets_out;
int po_agentsets_batch(po_handle h, const po_agentsets_params *p, const po_agentsets_in *in, const po_agentsets_out *out);         /* host pointers, synchronous */
int po_agentsets_batch_device(po_handle h, const po_agentsets_params *p, const po_agentsets_in *in, const po_agentsets_out *out);  /* device pointers, on the stream, no synchronisation */

/* ---- stop, wait, go: station-time plans that resume, sampled in time (csrc/po_stgo.hip, csrc/po_stsearch.hpp) ----
 * po_stplan_batch* may not resume after a stop, only because its one product is a v_limit row over arc length, which cannot carry a wait.  This stage runs the
 * same station-time search with resuming allowed and hands the plan over sampled at uniform TIME steps, in the layouts of po_trajectory_out: stop for a
 * pedestrian, let them clear, drive on.  out->states has the layout of every states array with N := Q, and with out->t it is a timed path po_dynamic_batch*
 * reads — intervals of positive duration and zero displacement included, so it checks the vehicle while it waits — and with out->v a profiled path
 * po_trajectory_batch* turns into agent records.  It writes no v_limit; po_stplan_batch* stays the stage for that.  The stage reads no map and works on a handle
 * without one.  The reference has no such stage.
 *
 * Definition (the bar is BIT equality).  The conventions are po_dynamic_batch's: every operation is one rounded IEEE double operation in the order written,
 * nothing contracted; sqrt and / are the correctly rounded ones; a comparison with a NaN is false; min and max as defined there.  n, row i, integer division:
 * as in po_stplan_batch.  The first ten fields of po_stgo_params are po_stplan_params' with the same ranges; t0, dts and Q are the sample times:
 * sample q < Q is at T_q = t0 + (double)q * dts.
 *   Not planned: status = 0 on po_stplan_batch's triggers (ok[b] == 0, or n < 2, or v0[b] not a finite value >= 0, or a non-finite x, y, z or s of rows < n, or
 *       M < 2), AND ADDITIONALLY when s_{i+1} < s_i for some i < n - 1: the sampler looks a state up by s, and a row that is not non-decreasing would make the
 *       answer depend on the search method.  (po_stplan_batch plans such a path; this is the one difference in what the two stages plan.)  The plan fields are
 *       as there (ok_out = 0, n_layers = 0, cost = DBL_MAX, station and cells rows -1); n_resumes = 0; every entry of the path's sample rows (states, v, a, t)
 *       is 0, every index -1, first_held = -1, end = 0.
 *   Stations, blocked cells, step table, search, choice, status, station, cells: the text of po_stplan_batch with the one clause "for k > 1, u' == 0 implies
 *       u == 0" deleted.  A predecessor at rest may have any successor: vp = v(j - u, 0) = 0, so acc = v(j, u) / dt <= a_max already bounds the pull-away, and
 *       waiting is costed by w_slow * c^2 like any slow edge.  Nothing else in the search changes.  No plan: status = 3, the samples are those of a path that
 *       is not planned, and the cells row is the map.
 *   n_resumes = the number of k in 2 .. n_layers with u_{k-1} == 0 and u_k > 0.
 *   Samples of a planned path, nl = n_layers.  V_0 = v0;  V_k = v(station[k], u_k) for k = 1 .. nl (0 when u_k == 0);  A_k = (V_k - V_{k-1}) / dt, the acc the
 *       search costed.  S_m is the s of station m.  For sample q, T = T_q, in this order:
 *       T < 0: the sample is row 0, with v = v0, a = 0, index = 0.
 *       Else kk = the largest k in 0 .. nl with (double)k * dt <= T: a T exactly on a layer time belongs to the later window.
 *       kk == nl: HELD.  The sample is the row of state station[nl] * stride, with v = V_nl, a = 0, index = that state.
 *       Else the edge is p = station[kk], j = station[kk+1], and tau = T - (double)kk * dt.
 *       j == p (standing): the sample is row p * stride, with v = 0, a = A_{kk+1}, index = p * stride.
 *       Else (moving):  sig = V_{kk+1} * tau;  sx = S_p + sig, then sx = sx > S_j ? S_j : sx;  i = the largest state index in [p * stride, j * stride - 1]
 *           with s_i <= sx (s is non-decreasing and s_{p * stride} = S_p <= sx, so the search method cannot change i);  ds = s_{i+1} - s_i;
 *           lam = ds > 0 ? (sx - s_i) / ds : 0, then lam = lam < 0 ? 0 : lam, then lam = lam > 1 ? 1 : lam;
 *           x = x_i + lam * (x_{i+1} - x_i), the same for y and k, and s = s_i + lam * ds;
 *           dz = z_{i+1} - z_i;  if dz > PI: dz = dz - TWO_PI, else if dz < -PI: dz = dz + TWO_PI  (the doubles 3.141592653589793 and 6.283185307179586);
 *           z = z_i + lam * dz, not wrapped again  (po_trajectory_batch's interpolation, character for character, with its own lam);
 *           v = V_{kk+1}, a = A_{kk+1}, index = i.
 *       out->t[b][q] = T for every sample of a planned path.
 *   first_held = the smallest q with kk == nl, Q when there is none (T_q is non-decreasing in q).
 *   end = 1 when first_held == Q: the samples end inside the plan.  Otherwise 2 when station[nl] is the path's last station (arrived), else 3 when u_nl == 0
 *       (the vehicle stands there), else 4: the plan ends AT SPEED before the samples do and the samples from first_held on repeat its last station — a vehicle
 *       that freezes where its plan ends, as po_trajectory_batch's status 3.
 *   Known and stated, not fixed: the speed is constant per window, which is the plan's own model, so v jumps at the layer times and a is the step the search
 *       costed, not a derivative of the samples.  po_stplan_batch's conservative sweep and the uncovered ground between two stations are inherited.  Feeding
 *       the samples to po_trajectory_batch* needs dts <= dt: further apart, two standing samples can have ground between them, which is that stage's end-state
 *       rule.  T = +inf (q * dts overflows) is held like any T >= nl * dt; T is never NaN because t0 and dts are finite.
 *   Decided while building: "aliasing" is po_trajectory_batch's overlap of byte ranges, every output array given over its full extent ([B], [B][17],
 *       [B][K][PO_ST_MAX_STATIONS], [B][Q][5], [B][Q]) against every input array given over its own (the agent lists are not among them); with B = 0 every
 *       extent is empty.  The extents are formed from K and Q only after their ranges are checked.
 * Return codes, both entries.  PO_ERR_INVALID: what po_stplan_batch refuses (NULL handle, struct or required pointer: states, v0, status, agents with B > 0;
 *   negative B, N, S, n_agents; S = 0 with B > 0; the ranges of the ten shared fields); t0 not finite; dts not finite or not > 0; Q < 1; with B > 0 a NULL
 *   out->states; an output that aliases an input.  The HOST entry refuses the lists po_dynamic_batch refuses; the DEVICE entry reads them clamped and never
 *   reads outside the buffers.  B = 0: PO_OK after those checks, nothing launched, nothing written.
 * `p`, `in->agents` (the struct) are host pointers in both entries.  Deterministic: no atomics, no scratch, and a path's results depend neither on the batch
 * size nor on its position in the batch.
 * po_default_stgo_params: po_default_stplan_params' values, then {0, 0.1, 81} — 81 samples at 10 Hz span the 8 s of K * dt.  A starting point nobody has tuned. */
typedef struct po_stgo_params {
    double dt;                   /* the ten fields of po_stplan_params, same meaning and ranges */
    int K;
    int stride;
    int U;
    double margin;
    double a_max, b_max;
    double v_max;
    double w_acc, w_slow;
    double t0, dts;              /* sample q is at T_q = t0 + (double)q * dts; t0 finite, dts > 0 and finite */
    int Q;                       /* >= 1 samples per path */
} po_stgo_params;
void po_default_stgo_params(po_stgo_params *p);
typedef struct po_stgo_in {      /* po_stplan_in without v_limit_in */
    int B, N;                    /* paths, rows per path (stride of the arrays) */
    const double *states;        /* [B][N][5] x, y, heading, k, s; s non-decreasing */
    const int    *n_states;      /* optional [B] (NULL: N) */
    const int    *ok;            /* optional [B] (NULL: all 1) */
    const double *v0;            /* [B] */
    const double *v_cap;         /* optional [B][N]: a per-state speed cap; negative or NaN: none */
    const int    *set_of;        /* optional [B] (NULL: set 0) */
    const po_agent_lists *agents;
} po_stgo_in;
typedef struct po_stgo_out {
    int    *status;              /* [B] 0 not planned, 1 planned and no cell blocked, 2 planned around blocked cells, 3 no plan */
    int    *ok_out;              /* optional [B]: status 1 or 2 */
    int    *n_layers;            /* optional [B] */
    double *cost;                /* optional [B] */
    int    *station;             /* optional [B][PO_ST_MAX_LAYERS + 1] */
    int    *cells;               /* optional [B][K][PO_ST_MAX_STATIONS] */
    int    *n_resumes;           /* optional [B]: times the plan pulls away after a window at rest */
    double *states;              /* [B][Q][5]: the states layout with N := Q */
    double *v, *a, *t;           /* optional [B][Q] */
    int    *index;               /* optional [B][Q]: the state a sample is anchored at; -1 without a plan */
    int    *first_held;          /* optional [B]: Q when no sample is held; -1 without a plan */
    int    *end;                 /* optional [B]: 0 no plan, 1 inside the plan, 2 held arrived, 3 held at rest, 4 held at speed */
} po_stgo_out;
int po_stgo_batch(po_handle h, const po_stgo_params *p, const po_stgo_in *in, const po_stgo_out *out);         /* host pointers, synchronous */
int po_stgo_batch_device(po_handle h, const po_stgo_params *p, const po_stgo_in *in, const po_stgo_out *out);  /* device pointers, on the stream, no synchronisation */

/* ---- speed QP: a jerk-limited s(t) inside a station-time plan's free tunnel (csrc/po_speedqp.hip) ----
 * po_stgo_batch* and po_stplan_batch* decide — pass, yield, stop, wait, go — on windows of dt with constant speed per window, which no controller can track.
 * This stage takes the plan (station, n_layers) and the cell map (cells) they leave, turns the plan's gaps into a tunnel lo_q <= s(T_q) - S_0 <= hi_q at the
 * sample times, and solves a piecewise-jerk QP inside it per path: the search keeps the decision, the QP makes the motion.  The result leaves in the layouts of
 * po_stgo_out / po_trajectory_out, so stgo -> speed QP -> dynamic and stgo -> speed QP -> trajectory -> agent sets stay on one stream.  No agents and no map
 * are read; the stage works on a handle without a map.  The reference has no such stage.
 *
 * Definition (the bar is BIT equality).  The conventions are po_dynamic_batch's: every operation is one rounded IEEE double operation in the order written,
 * nothing contracted; sqrt and / are the correctly rounded ones; a comparison with a NaN is false; min(a, b) = b < a ? b : a; max(a, b) = b > a ? b : a.
 * n, row i, M, S_m, Vc_m: as in po_stplan_batch (from dt, K, stride, v_max and v_cap).  T_q = (double)q * dts, q < Q; h = dts; i1 = 1 / h, i2 = i1 / h, i3 = i2 / h.
 *   Not run: status = 0 on po_stgo_batch's "not planned" triggers (ok[b] == 0, n < 2, v0[b] not a finite value >= 0, a non-finite x, y, z or s of rows < n,
 *       s_{i+1} < s_i for some i < n - 1, M < 2), and when nl = n_layers[b] clamped into [0, K] is < 1, when station[b][k], k = 0 .. nl, each clamped into
 *       [0, PO_ST_MAX_STATIONS - 1], has station[k+1] < station[k] for some k < nl or station[nl] > M - 1, and when ref_states[b][q][4] is not finite for
 *       some q < n_q.  Then iters = n_fact = n_q = 0, r_prim = r_dual = 0, every entry of the path's sample rows (states, v, a, jerk, t, lo, hi) is 0, every index -1.
 *   n_q = the number of q < Q with T_q <= (double)nl * dt (>= 1).  Samples q < n_q are the unknowns x_q = s(T_q) - S_0; write n for n_q below.
 *   Tunnel.  kk = the largest k in 0 .. nl with (double)k * dt <= T_q.  The windows of sample q are kk - 1 when kk >= 1 and T_q == (double)kk * dt, then kk, each
 *       only when <= nl - 1.  For a window w, p = station[w], j = station[w+1]: lo_m = 1 + the largest m < p with cells[b][w][m] >= 0, 0 when there is none;
 *       hi_m = -1 + the smallest m in j + 1 .. M - 1 with cells[b][w][m] >= 0, M - 1 when there is none (cells NULL: there is none).  lo_q = the first window's
 *       S_{lo_m} - S_0, then max(lo_q, the second's); hi_q likewise with min and S_{hi_m} - S_0.  lo_0 = hi_0 = 0.
 *       C_q, q < n - 1: w = min(kk, nl - 1); c = Vc_{station[w]}, then c = min(c, Vc_m) for m = station[w] + 1 .. station[w+1], ascending.
 *   Rows, in four classes.  d_r = x_{r+1} - x_r (r = 0 .. n - 2);  e_r = d_r - d_{r-1} with d_{-1} = 0;  f_r = e_{r+1} - e_r.
 *       position  r = 0 .. n - 1:  x_r             in [lo_r, hi_r]
 *       velocity  r = 0 .. n - 2:  d_r * i1        in [0, C_r]
 *       accel.    r = 0 .. n - 2:  e_r * i2        in [-b_max, a_max], row 0 in [-b_max + c0, a_max + c0] with c0 = v0 * i1 (its constant moved into the bounds)
 *       jerk      r = 1 .. n - 3:  f_r * i3        in [-j_max, j_max]
 *       A x is these values.  A^T w, for row values w (0 for a row that does not exist):  pj_r = wj_r * i3;  tj_r = pj_{r-1} - pj_r;  ta_r = wa_r * i2 + tj_r;
 *       tb_r = ta_r - ta_{r+1} (ta_{n-1} = 0);  tv_r = wv_r * i1 + tb_r, r = 0 .. n - 2;  (A^T w)_q = wp_q + (tv_{q-1} - tv_q) with tv_{-1} = tv_{n-1} = 0.
 *       A row is an EQUALITY row when its l and u have the same 64 bits; rho_r = 1e3 * rho on those, rho elsewhere (rho: the path's current step).
 *   Cost.  sum w_s (x_q - r_q)^2 + w_a (e_r * i2 - [r == 0] c0)^2 + w_j (f_r * i3)^2 with r_q = ref_states[b][q][4] - S_0.  In OSQP's form, with
 *       tws = 2 * w_s, twa = 2 * w_a, twj = 2 * w_j:  P x = tws * x + A^T(0, 0, twa * (A x)_a, twj * (A x)_j);  qv = -(tws * r + A^T(0, 0, (twa * c0 at row 0), 0)).
 *   Matrix.  Column c of K = P + sigma I + A^T diag(rho) A is A^T(gp * (A u)_p, rho_r * (A u)_v, (rho_r + twa) * (A u)_a, (rho_r + twj) * (A u)_j) for the unit
 *       vector u of c, with gp = rho_r + (tws + sigma); its entries c .. c + 3 are the lower band K0 .. K3 of column c (0 behind row n - 1).
 *       Factor, j = 0 .. n - 1 ascending, terms with a negative index left out:  D_j = ((K0_j - (L1_{j-1} * D_{j-1}) * L1_{j-1}) - (L2_{j-2} * D_{j-2}) * L2_{j-2})
 *       - (L3_{j-3} * D_{j-3}) * L3_{j-3};  c1 = (K1_j - (L2_{j-1} * D_{j-1}) * L1_{j-1}) - (L3_{j-2} * D_{j-2}) * L2_{j-2};  c2 = K2_j - (L3_{j-1} * D_{j-1}) * L1_{j-1};
 *       L1_j = c1 / D_j, L2_j = c2 / D_j, L3_j = K3_j / D_j  (Lk_j is the entry (j + k, j)).
 *       Solve K xt = rhs:  yv_q = ((rhs_q - L3_{q-3} * yv_{q-3}) - L2_{q-2} * yv_{q-2}) - L1_{q-1} * yv_{q-1}, ascending;  w_q = yv_q / D_q;
 *       xt_q = ((w_q - L3_q * xt_{q+3}) - L2_q * xt_{q+2}) - L1_q * xt_{q+1}, descending, terms with an index >= n left out.
 *   Iteration, from x = 0, z = 0, y = 0, rho = p->rho, n_fact = 1, for it = 1 .. max_iter, om = 1 - alpha:
 *       rhs = (sigma * x - qv) + A^T(rho_r * z_r - y_r);  xt as above;  zt = A xt;  x = alpha * xt + om * x;  per row zr = alpha * zt_r + om * z_r,
 *       zc = zr + y_r / rho_r, z_r = min(max(zc, l_r), u_r) (that is: l_r > zc ? l_r : zc, then u_r < that ? u_r : that), y_r = y_r + rho_r * (zr - z_r).
 *       When it % check_every == 0 or it == max_iter:  a norm |.| is the largest |v| of its entries COMPARED AS 64-BIT PATTERNS, so it depends on no order
 *       and a NaN outranks every number.  r_prim = |A x - z|, r_dual = |(P x + qv) + A^T y|, mp = max(|A x|, |z|), md = max(max(|P x|, |A^T y|), |qv|),
 *       ep = eps_abs + eps_rel * mp, ed = eps_abs + eps_rel * md.  r_prim <= ep and r_dual <= ed: status 1, stop.  Else it == max_iter: status 2, stop.
 *       Else with adaptive_rho: rn = rho * sqrt((r_prim / mp) / (r_dual / md)), rn = 1e-6 > rn ? 1e-6 : rn, rn = 1e6 < rn ? 1e6 : rn; when rn > 5 * rho or
 *       rn < rho / 5: rho = rn, the matrix is factorised again and n_fact counts it.  iters = the it of the stop; r_prim, r_dual: the last check's.
 *   n_q == 1: status 1 without iterations (iters = n_fact = 0, residuals 0), x_0 = 0.
 *   Samples from the iterate x (not z).  sq = S_0 + x_q;  sx = sq < s_0 ? s_0 : sq, then sx = sx > s_{n-1} ? s_{n-1} : sx;  i = the result of the bisection
 *       lo = 0, hi = n - 1, while hi - lo > 1: mid = lo + (hi - lo) / 2, s_mid <= sx ? lo = mid : hi = mid — the largest i <= n - 2 with s_i <= sx, and state 0
 *       for a NaN;  ds, lam, x, y, k, s, dz and z: po_stgo_batch's moving sample, character for character;  index = i.
 *       v_0 = v0, v_q = (x_q - x_{q-1}) / h;  a_q = (v_{q+1} - v_q) / h, 0 at q = n - 1;  jerk_q = (a_{q+1} - a_q) / h, 0 at q >= n - 2.  Samples q >= n_q (HELD)
 *       repeat sample n_q - 1's row, index, v, lo and hi with a = jerk = 0 — po_stgo_batch's held rule.  t_q = T_q for every sample of a path that ran.
 *   Known and stated, not fixed: there is no previous acceleration a0 (a_0 is bounded against v0 only), no primal-infeasibility certificate (a tunnel that v0
 *       cannot meet ends as status 2 with the iterate written), the caps follow the plan's windows and not the smoothed s, no equilibration and no polish,
 *       agents are po_agent's discs as in the planners, the entries are not meant for graph capture, and po_plan_batch* does not call the stage.
 *   Decided while building: the norms compare bit patterns (above) so that a NaN cannot make them depend on an order; acceleration row 0 keeps A linear by moving
 *       c0 into its bounds and into qv; the matrix is DEFINED through the operators on unit vectors, so its bits need no second formula; the held samples
 *       repeat lo and hi too; "aliasing" is po_stgo_batch's overlap of byte ranges, every output over its full extent ([B], [B][Q][5], [B][Q]) against every
 *       input over its own ([B][N][5], [B], [B][N], [B][PO_ST_MAX_LAYERS + 1], [B][K][PO_ST_MAX_STATIONS], [B][Q][5]), formed after K and Q are checked.
 * Return codes, both entries.  PO_ERR_INVALID: a NULL handle, struct or required pointer (with B > 0: states, v0, station, n_layers, ref_states, out->status,
 *   out->states); negative B or N; dt, v_max, dts, a_max, b_max, j_max, rho, sigma not finite or not > 0; K outside 1 .. PO_ST_MAX_LAYERS; stride < 1; Q outside
 *   2 .. PO_SQP_MAX_SAMPLES; a weight negative or not finite, or w_s + w_a + w_j not > 0; alpha not inside (0, 2); eps_abs or eps_rel negative or not finite;
 *   max_iter < 1; check_every < 1; adaptive_rho not 0 or 1; an output that aliases an input.  The HOST entry also refuses an n_layers[b] outside [0, K] and, on a
 *   path with n_layers[b] >= 1, a station[b][k], k <= n_layers[b], outside [0, PO_ST_MAX_STATIONS - 1]; the DEVICE entry reads them clamped (above) and never
 *   reads outside the buffers.  B = 0: PO_OK after those checks, nothing launched, nothing written.
 * `p` is a host pointer in both entries.  Deterministic: no atomics, no scratch, and a path's results depend neither on the batch size nor on its position in it.
 * po_default_speedqp_params: po_default_stgo_params' dt, K, stride, v_max, dts and Q; limits 2 / 3 / 4; weights 1 / 1 / 1; then 0.1, 1e-6, 1.6, 1e-4, 1e-4,
 *   2000, 25, 1.  A starting point nobody has tuned. */
#define PO_SQP_MAX_SAMPLES 256
typedef struct po_speedqp_params {
    double dt;                   /* the plan's grid: the planner's dt, K, stride and v_max */
    int K;
    int stride;
    double v_max;
    double dts;                  /* the sample grid: the planner's dts and Q, with t0 = 0 */
    int Q;                       /* 2 .. PO_SQP_MAX_SAMPLES */
    double a_max, b_max, j_max;  /* acceleration in [-b_max, a_max], |jerk| <= j_max */
    double w_s, w_a, w_j;        /* weights of the distance to the plan's samples, of acceleration and of jerk */
    double rho, sigma, alpha, eps_abs, eps_rel;
    int max_iter, check_every, adaptive_rho;
} po_speedqp_params;
void po_default_speedqp_params(po_speedqp_params *p);
typedef struct po_speedqp_in {
    int B, N;                    /* paths, rows per path (stride of the arrays) */
    const double *states;        /* [B][N][5] x, y, heading, k, s; s non-decreasing */
    const int    *n_states;      /* optional [B] (NULL: N) */
    const int    *ok;            /* optional [B] (NULL: all 1): the planner's ok_out */
    const double *v0;            /* [B] */
    const double *v_cap;         /* optional [B][N] */
    const int    *station;       /* [B][PO_ST_MAX_LAYERS + 1]: the planner's out->station */
    const int    *n_layers;      /* [B]: the planner's out->n_layers */
    const int    *cells;         /* optional [B][K][PO_ST_MAX_STATIONS]: the planner's out->cells; NULL: nothing is blocked */
    const double *ref_states;    /* [B][Q][5]: the planner's samples at the same dts and Q with t0 = 0; column 4 is read */
} po_speedqp_in;
typedef struct po_speedqp_out {
    int    *status;              /* [B] 0 not run, 1 converged, 2 max_iter reached (the iterate is written) */
    int    *iters, *n_fact;      /* optional [B] */
    double *r_prim, *r_dual;     /* optional [B]: the residuals of the last check */
    int    *n_q;                 /* optional [B]: samples in the QP */
    double *states;              /* [B][Q][5] */
    double *v, *a, *jerk, *t;    /* optional [B][Q] */
    double *lo, *hi;             /* optional [B][Q]: the tunnel, relative to S_0 */
    int    *index;               /* optional [B][Q] */
} po_speedqp_out;
int po_speedqp_batch(po_handle h, const po_speedqp_params *p, const po_speedqp_in *in, const po_speedqp_out *out);         /* host pointers, synchronous */
int po_speedqp_batch_device(po_handle h, const po_speedqp_params *p, const po_speedqp_in *in, const po_speedqp_out *out);  /* device pointers, on the stream, no synchronisation */

/* Test/diagnostic entry: Map::getObstacleDistance at `n` world positions xy[n][2] (host pointers); inside[n] = Map::isInside. */
int po_map_sample(po_handle h, int n, const double *xy, double *dist, int *inside);

/* Test/diagnostic entry: run only the device assembly and return the QP data in the REFERENCE
 * row order: l,u [B][m]; dyn [B][N-1][3] = per-transition data-dependent A entries
 * (KP/KPC: ds, -k^2*ds, ds ; K: -ds*k^2, ds, ds/L/cos^2) ; host pointers. */
int po_assemble_batch(po_handle h, const po_batch_in *in, double *l, double *u, double *dyn);

/* Test/diagnostic entry: the per-path equilibration block [B][64] the solve kernel consumes
 * (layout in csrc/po_scale.hpp: W = E^2/c per row class, E, sigma/(c D^2) and c*D per variable class, c). */
int po_scaling_batch(po_handle h, const po_batch_in *in, double *out);

/* Kernel time (ms) of the last timed launch sequence on this handle, measured with hipEvents on the handle's stream (valid after the
 * stream has been synchronised): po_solve_batch* (equilibration + solve launches + polish) or po_smooth_batch*.  After po_plan_batch*, which
 * issues several of them, it is the LAST such sequence of the chain (the path QP of the last keep-group), not the whole call. */
int po_last_kernel_ms(po_handle h, float *ms);
/* Where the last solve spent its time, ms8[8] (hipEvents on the handle's stream + host wall clock; valid after the call returned / the stream was synchronised):
 *   after po_solve_batch (host pointers: the caller's arrays are packed into a pinned staging block on several host threads while the slices already packed travel
 *   over PCIe, one D2H into a pinned block, threaded unpack): [0] pack + H2D, [1] the solve (= po_last_kernel_ms), [2] D2H, [3] host pack alone, [4] host unpack;
 *   with po_params.refine = 2 (either entry): [5] equilibration + warm-start launches, [6] the Newton launch, [7] what follows it: the fallback launch when a path needs it (refine_chain = 3: always), status sweep. */
int po_last_phase_ms(po_handle h, float *ms8);

const char *po_strerror(int code);
const char *po_last_hip_error(void);
/* "po_hip <abi> (gfx950)"; PO_ABI_VERSION is bumped whenever a struct layout, an entry point or the meaning of a field changes (5: round 5, see po_params.refine;
 * 6: round 6, po_info.status_refine / status_polish may be PO_NOT_AVAILABLE; po_create refuses refine_rounds + refine_extra_rounds >= 32; 7: po_occupancy,
 * po_distance_map_batch*, po_set_map_occupancy*, po_get_map, po_debug_get "map_ptr").  The map-stack entries
 * (po_set_map_stack*, po_set_map_assignment*, po_get_map_layer, po_map_sample_layer, po_debug_get "map_layers") were ADDED under 7: no struct layout, no existing
 * entry and no field's meaning changed, so a binding written against 7 drives this library unchanged; one that needs the new entries looks the symbols up.  The
 * obstacle-list entries (po_obstacle, po_obstacle_lists, po_rasterize_batch*, po_set_map_stack_obstacles*) and the static-world entries (po_rings, po_scene, po_set_world_occupancy*, po_rasterize_scene_batch*, po_set_map_stack_scene*,
 * po_debug_get "world_cells") and the score-and-select entries (po_select_params, po_select_in, po_select_out, po_default_select_params, po_select_batch*) and
 * the speed-profile entries (po_speed_params, po_speed_in, po_speed_out, po_default_speed_params, po_speed_batch*) and the moving-obstacle entries (po_agent, po_agent_lists, po_dynamic_params, po_dynamic_in, po_dynamic_out,
 * po_default_dynamic_params, po_dynamic_batch*) and the station-time entries (po_stplan_params, po_stplan_in, po_stplan_out, po_default_stplan_params,
 * po_stplan_batch*) and the corridor-nudge entries (po_nudge_params, po_nudge_in, po_nudge_out, po_default_nudge_params, po_nudge_batch*) and the timed-trajectory
 * entries (po_trajectory_params, po_trajectory_in, po_trajectory_out, po_default_trajectory_params, po_trajectory_batch*) and the agent-set
 * entries (po_agentsets_params, po_agentsets_in, po_agentsets_out, po_default_agentsets_params, po_agentsets_batch*) and the stop-wait-go entries (po_stgo_params, po_stgo_in, po_stgo_out,
 * po_default_stgo_params, po_stgo_batch*) and the speed-QP entries (po_speedqp_params, po_speedqp_in, po_speedqp_out, po_default_speedqp_params,
 * po_speedqp_batch*, PO_SQP_MAX_SAMPLES) were added under 7 by
 * the same rule.  A binding should compare
 * the number in po_version() with the PO_ABI_VERSION it was written against before it passes a struct (path_optimizer_amd/binding.py does). */
#define PO_ABI_VERSION 7
const char *po_version(void);

#ifdef __cplusplus
}
#endif
#endif /* PO_HIP_H_ */
