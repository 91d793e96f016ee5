// po_map.hpp — obstacle-distance map sampling and the post-solve collision check, gfx950.
//
// Reference: PathOptimizationNS::Map::{getObstacleDistance,isInside} (src/tools/Map.cpp:16-26),
// CollisionChecker::isSingleStateCollisionFree{,Improved} (src/tools/collision_checker.cpp:17-59),
// CarGeometry (src/tools/car_geometry.cpp:38-72), the output loop of PathOptimizer::optimizePath
// (src/path_optimizer/path_optimizer.cpp:183-200).
// grid_map (ROS package grid_map_core, NOT in /root/reference, un-pinned) is restated from its published sources:
// GridMap::isInside -> checkIfPositionWithinMap, GridMap::atPosition(INTER_LINEAR) -> atPositionLinearInterpolated with the
// nearest-cell fallback, index/position conversions of GridMapMath.cpp.  "parity unpinned" for that part.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/po_hip.h"
#include "../../include/po_pmath.h"  // portable sin / cos / atan2: the same IEEE operation sequence as the oracle's portable-math mode (bit-exact map stages)

namespace po {

struct DevMap {
    const float *d;  // column-major [sy][sx]
    int sx, sy;
    double res, px, py;
};
// The handle's map STACK (po_set_map_stack*): M layers of one geometry, layer k at d + k * stride, and which layer instance b of a batch reads.
// A view: nothing here is owned.  M = 1 with pos == layer_of == nullptr is the single map of po_set_map.
struct DevMaps {
    const float *d;       // layer 0 (nullptr: no map installed)
    int sx, sy;
    double res, px, py;   // px, py: centre of every layer when pos == nullptr
    int M;
    size_t stride;        // elements per layer (sx * sy)
    const double *pos;    // device [M][2]: centre of each layer, or nullptr
    const int *layer_of;  // device [n_assign]: layer of instance b, or nullptr = every instance reads layer 0
    int n_assign;
};
struct DevCar {  // CollisionChecker's CarGeometry, built on the host exactly like car_geometry.cpp:38-56
    double bx, br;            // bounding circle (local x, radius); local y = 0
    double cx[6], cy[6], cr[6];
    int enable;
};

// corridor-bounds producer launch arguments (po_post.hip)
struct DevBounds {
    int B, N, K;
    const double *ref_x, *ref_y, *ref_z, *ref_s;
    const int *n_points;
    const double *knot_s, *knot_x, *knot_y;
    const int *n_knots;
    double d[4], radius;
    double *coef;  // [B][2][6][K]: per spline a, b, c + 3K scratch
};

// re-sampling / DP search launch arguments (po_post.hip), SURVEY.md §8f-4
struct DevSpline {
    int B, K;
    const double *knot_s, *knot_x, *knot_y;
    const int *n_knots;
    const double *length;
    double *coef;  // [B][2][6][K] as in DevBounds
};
struct DevSearch {
    double range, long_spacing, lat_spacing;
    const double *start;  // [B][3]
    int L;                // stride / cap of the per-layer outputs
    double *layer_s, *lb, *ub, *l0;
    int *n_layers;
};
struct DevResample {
    double ds_small, ds_large;
    int dynamic, N;
    double *x, *y, *z, *k, *s;
    int *n_points;
};

// plumbing of po_plan_batch (po_post.hip kernels, po_plan.cpp orchestration)
struct PlanGate {
    int B, mode;
    int *stage;
    int *cnt;               // the count array the next stage reads (n_points / n_layers / n_valid): zeroed for failed instances
    const int *cnt2;        // mode 1: n_samples of the B-spline stage
    const po_info *info;    // modes 1, 3, 6: the QP info to test
    const double *s; int stride;  // mode 1: result_s (for length = s.back() + 3)
    double *length;         // modes 1, 4: length handed to the next spline stage
    const double *init; const int *ok;  // mode 4
    const double *start, *goal;         // mode 5: [B][4], [B][3]
    const double *ref_s; int ref_stride;  // mode 5: reference arc lengths (keep_control_steps)
    double *x0, *goal_z; int *keep;     // mode 5 outputs
    double *start3;         // mode 0: start [B][3] for the search
};
struct PlanRows {
    int G, N, Ng;
    const int *idx;  // [G] instance of each group row
    const double *ref_x, *ref_y, *ref_z, *ref_k, *ref_s, *bounds, *x0, *goal_z;
    const int *n_valid;
    double *g_x, *g_y, *g_z, *g_k, *g_s, *g_bounds, *g_x0, *g_goal;
    int *g_n;
    double *g_states; po_info *g_info;  // solve outputs of the group
    double *states; po_info *info;      // [B][N][5], [B]
};

// score-and-select launch arguments (po_select.hip): po_select_in / po_select_out, the knobs of po_select_params, and the handle's scratch
struct DevSelect {
    int B, N, G, Np, goal_stride;
    const double *states; const int *n_states, *ok; const double *goal;
    const int *group_start;  // the caller's table [G + 1], unvalidated
    const double *prev_states; const int *prev_n;
    double w[PO_N_FEAT], d_safe, min_clearance, max_kmax, max_goal_dist;
    int *gs;                 // scratch [G + 1]: the table as the kernels read it (clamped, non-decreasing)
    double *feat, *cost;     // cost is never null here (the handle's scratch when the caller gave none)
    int *best; double *best_cost; int *n_feasible; double *sel_states; int *sel_n;
};

// speed-profile launch arguments (po_speed.hip): po_speed_in / po_speed_out, the knobs of po_speed_params, A = mu * 9.8 and R = max_curvature_rate
struct DevSpeed {
    int B, N, use_map;
    const double *states; const int *n_states, *ok; const double *v0, *v_end, *v_limit;
    double v_max, a_lat_max, a_max, b_max, clear_v0, clear_gain, A, R;
    double *v, *a, *t, *total_time;  // v also carries W and w between the kernels; t and total_time may be null
    int *status;
};

// moving-obstacle launch arguments (po_dynamic.hip): po_dynamic_in / po_dynamic_out with the lists of po_agent_lists flattened, and the two
// knobs of po_dynamic_params.  Every output but status may be null.
struct DevDynamic {
    int B, N, S, n_agents;
    const double *states; const int *n_states, *ok; const double *t; const int *set_of;
    const po_agent *agents; const int *first;
    const double *v_limit_in;
    double margin, stop_distance;
    int *status, *ok_out; double *gap_min; int *first_state, *first_agent, *stop_state; double *first_time, *gap, *v_limit;
};

// station-time planning launch arguments (po_stplan.hip): po_stplan_in / po_stplan_out with the lists of po_agent_lists flattened, the fields
// of po_stplan_params, and Mb = min((N - 1) / stride + 1, PO_ST_MAX_STATIONS), the bound on the stations of a path that sizes the LDS.  Every output but status
// may be null.  DevStSearch is what the phases of po_stsearch.hpp read and write: the part po_stplan.hip and po_stgo.hip share.
struct DevStSearch {
    int B, N, S, n_agents;
    const double *states; const int *n_states, *ok; const double *v0, *v_cap; const int *set_of;
    const po_agent *agents; const int *first;
    double dt; int K, stride, U, Mb; double margin, a_max, b_max, v_max, w_acc, w_slow;
    int *status, *ok_out, *n_layers; double *cost; int *station, *cells;
};
struct DevStplan : DevStSearch {
    const double *v_limit_in;
    double *v_limit;
};

// stop-wait-go launch arguments (po_stgo.hip): the search's, the sample times of po_stgo_params (sample q at t0 + q * dts, q < Q) and the
// sample outputs of po_stgo_out.  Every output but status and o_states may be null.
struct DevStgo : DevStSearch {
    double t0, dts; int Q;
    int *n_resumes; double *o_states, *o_v, *o_a, *o_t; int *index, *first_held, *end;
};

// speed-QP launch arguments (po_speedqp.hip): po_speedqp_in / po_speedqp_out and the fields of po_speedqp_params.  Every output but status
// and o_states may be null; n_states, ok, v_cap and cells may be null.
struct DevSpeedQp {
    int B, N, K, stride, Q;
    double dt, v_max, dts, a_max, b_max, j_max, w_s, w_a, w_j, rho, sigma, alpha, eps_abs, eps_rel;
    int max_iter, check_every, adaptive_rho;
    const double *states; const int *n_states, *ok; const double *v0, *v_cap; const int *station, *n_layers, *cells; const double *ref_states;
    int *status, *iters, *n_fact; double *r_prim, *r_dual; int *n_q; double *o_states, *o_v, *o_a, *o_jerk, *o_t, *o_lo, *o_hi; int *index;
};

// corridor-nudge launch arguments (po_nudge.hip): po_nudge_in / po_nudge_out with the lists of po_agent_lists flattened, the fields of
// po_nudge_params, and d and radius as DevBounds carries them.  bounds_in and bounds never alias.  Every output but status and bounds may be null.
struct DevNudge {
    int B, N, W, S, n_agents, skip_states;
    const double *ref_x, *ref_y, *ref_z; const int *n_points, *ok; const double *t, *bounds_in; const int *set_of;
    const po_agent *agents; const int *first; const int *side_prev;
    double d[4], radius, margin, t_before, t_after, min_width;
    int *status, *ok_out; double *bounds; int *side, *first_blocked_state, *first_blocked_agent; double *width_min;
};

// timed-trajectory launch arguments (po_trajectory.hip): po_trajectory_in / po_trajectory_out and the fields of po_trajectory_params
// (D = n_discs, P = agent_pts).  Every output but status and o_states may be null; agents is null exactly when D == 0.
struct DevTrajectory {
    int B, N, K, D, P, stride, flags;
    const double *states; const int *n_states, *ok; const double *v, *t;
    double t0, dt, off[PO_TRAJ_MAX_DISCS], rad[PO_TRAJ_MAX_DISCS];
    int *status; double *o_states, *o_v, *o_a, *o_t; int *index, *first_held; po_agent *agents;
};

// agent-set launch arguments (po_agentsets.hip): po_agentsets_in / po_agentsets_out and the fields of po_agentsets_params; the two sources
// side by side (S[1] = 0: source 1 contributes nothing).  t, pool_of, owner, o_set_of, src_index and total may be null; o_agents is null only with capacity 0.
struct DevAgentSets {
    int B, N, capacity, owner_div;
    const double *states; const int *n_states, *ok; const double *t; const int *pool_of, *owner;
    const po_agent *agents[PO_SETS_SOURCES]; const int *first[PO_SETS_SOURCES]; int n_agents[PO_SETS_SOURCES], S[PO_SETS_SOURCES];
    double reach, t_before, t_after, win_lo, win_hi;
    po_agent *o_agents; int *o_first, *count, *status, *o_set_of, *src_index; long long *total;
};

#ifdef PO_MAP_DEVICE_CODE  // kernels and device functions: po_kernels.hip only (po_capi.cpp needs just the structs)
// Layer k of the stack as a DevMap.  k is clamped into [0, M - 1] HERE, where it is read: a table that arrived through a device pointer was never validated, and a
// bad entry must select a wrong layer, never an address outside the stack.
__device__ __forceinline__ DevMap map_layer(const DevMaps &s, int k) {
    k = k < 0 ? 0 : (k >= s.M ? s.M - 1 : k);
    DevMap m{s.d + (size_t)k * s.stride, s.sx, s.sy, s.res, s.px, s.py};
    if (s.pos) { m.px = s.pos[2 * (size_t)k]; m.py = s.pos[2 * (size_t)k + 1]; }
    return m;
}
// The map instance b reads.  Every caller runs one workgroup (or wave) per instance and passes the block's instance: b is wave-uniform, so the table entry, the
// positions and the layer base are scalar loads and the DevMap stays in scalar registers, as the by-value kernel argument did.
__device__ __forceinline__ DevMap map_of(const DevMaps &s, int b) {
    return map_layer(s, (s.layer_of && b >= 0 && b < s.n_assign) ? s.layer_of[b] : 0);
}
// checkIfPositionWithinMap (GridMapMath.cpp): t = -(p - mapPos - 0.5*len); 0 <= t < len on both axes
__device__ __forceinline__ bool map_inside(const DevMap &m, double x, double y) {
    const double lx = m.sx * m.res, ly = m.sy * m.res;
    const double tx = -(__dsub_rn(__dsub_rn(x, m.px), __dmul_rn(0.5, lx)));
    const double ty = -(__dsub_rn(__dsub_rn(y, m.py), __dmul_rn(0.5, ly)));
    return tx >= 0.0 && ty >= 0.0 && tx < lx && ty < ly;
}
// getIndexFromPosition: idx = (int)( -((p - 0.5*len - mapPos) / res) )   (C++ double->int conversion truncates)
__device__ __forceinline__ void map_index(const DevMap &m, double x, double y, int &ix, int &iy) {
    const double lx = m.sx * m.res, ly = m.sy * m.res;
    ix = (int)(-(__dsub_rn(__dsub_rn(x, __dmul_rn(0.5, lx)), m.px) / m.res));
    iy = (int)(-(__dsub_rn(__dsub_rn(y, __dmul_rn(0.5, ly)), m.py) / m.res));
}
__device__ __forceinline__ bool map_index_ok(const DevMap &m, int ix, int iy) { return ix >= 0 && iy >= 0 && ix < m.sx && iy < m.sy; }
// getPositionFromIndex: p = (mapPos + (0.5*len - 0.5*res)) + res * (-idx); leaves p untouched when idx is out of range
__device__ __forceinline__ void map_position(const DevMap &m, int ix, int iy, double &x, double &y) {
    if (!map_index_ok(m, ix, iy)) return;
    const double lx = m.sx * m.res, ly = m.sy * m.res;
    x = __dadd_rn(__dadd_rn(m.px, __dsub_rn(__dmul_rn(0.5, lx), __dmul_rn(0.5, m.res))), __dmul_rn(m.res, (double)(-ix)));
    y = __dadd_rn(__dadd_rn(m.py, __dsub_rn(__dmul_rn(0.5, ly), __dmul_rn(0.5, m.res))), __dmul_rn(m.res, (double)(-iy)));
}
// GridMap::atPosition(layer, p, INTER_LINEAR) for a position that isInside (the only way the reference calls it)
__device__ __forceinline__ double map_at_linear(const DevMap &m, double x, double y) {
    int i0x, i0y;
    map_index(m, x, y, i0x, i0y);
    double ptx = 0, pty = 0;
    map_position(m, i0x, i0y, ptx, pty);
    int ix[4], iy[4], sh[4];
    ix[0] = i0x; iy[0] = i0y;
    bool up;
    if (x >= ptx) { ix[1] = i0x - 1; iy[1] = i0y; up = true; } else { ix[1] = i0x + 1; iy[1] = i0y; up = false; }
    if (y >= pty) {
        ix[2] = i0x; iy[2] = i0y - 1;
        if (up) { sh[0] = 0; sh[1] = 1; sh[2] = 2; sh[3] = 3; } else { sh[0] = 1; sh[1] = 0; sh[2] = 3; sh[3] = 2; }
    } else {
        ix[2] = i0x; iy[2] = i0y + 1;
        if (up) { sh[0] = 2; sh[1] = 3; sh[2] = 0; sh[3] = 1; } else { sh[0] = 3; sh[1] = 2; sh[2] = 1; sh[3] = 0; }
    }
    ix[3] = ix[1]; iy[3] = iy[2];
    const long long nbuf = (long long)m.sx * m.sy;
    float f[4];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int jx = 0, jy = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) if (sh[i] == k) { jx = ix[k]; jy = iy[k]; }
        // the library tests the LINEAR index (size_t) against [0, size]: a row index of -1 wraps into the previous column
        const long long lin = (long long)jy * m.sx + jx;
        if (lin < 0 || lin > nbuf) ok = false;
        f[i] = (lin >= 0 && lin < nbuf) ? m.d[lin] : 0.0f;  // (lin == size would read one past the buffer in the library)
    }
    if (ok) {
        int jx = 0, jy = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) if (sh[0] == k) { jx = ix[k]; jy = iy[k]; }
        map_position(m, jx, jy, ptx, pty);
        const double rx = __dsub_rn(x, ptx) / m.res, ry = __dsub_rn(y, pty) / m.res;
        const double fx = __dsub_rn(1.0, rx), fy = __dsub_rn(1.0, ry);
        double v = __dmul_rn(__dmul_rn((double)f[0], fx), fy);
        v = __dadd_rn(v, __dmul_rn(__dmul_rn((double)f[1], rx), fy));
        v = __dadd_rn(v, __dmul_rn(__dmul_rn((double)f[2], fx), ry));
        v = __dadd_rn(v, __dmul_rn(__dmul_rn((double)f[3], rx), ry));
        return (double)(float)v;  // the library returns float
    }
    // INTER_NEAREST fallback
    return map_index_ok(m, i0x, i0y) ? (double)m.d[(long long)i0y * m.sx + i0x] : 0.0;
}
// Map::getObstacleDistance (Map.cpp:16-22)
__device__ __forceinline__ double map_distance(const DevMap &m, double x, double y) { return map_inside(m, x, y) ? map_at_linear(m, x, y) : 0.0; }

// CollisionChecker::isSingleStateCollisionFreeImproved (collision_checker.cpp:42-59)
__device__ __forceinline__ bool collision_free(const DevMap &m, const DevCar &c, double x, double y, double z) {
    const double cz = po_pcos(z), sz = po_psin(z);
    // local2Global (tools.cpp:50-55): x = tx cos - ty sin + rx ; y = tx sin + ty cos + ry
    const double bx = __dadd_rn(__dsub_rn(__dmul_rn(c.bx, cz), __dmul_rn(0.0, sz)), x);
    const double by = __dadd_rn(__dadd_rn(__dmul_rn(c.bx, sz), __dmul_rn(0.0, cz)), y);
    if (!map_inside(m, bx, by)) return false;
    if (!(map_at_linear(m, bx, by) < c.br)) return true;
#pragma unroll 1
    for (int k = 0; k < 6; ++k) {
        const double gx = __dadd_rn(__dsub_rn(__dmul_rn(c.cx[k], cz), __dmul_rn(c.cy[k], sz)), x);
        const double gy = __dadd_rn(__dadd_rn(__dmul_rn(c.cx[k], sz), __dmul_rn(c.cy[k], cz)), y);
        if (!map_inside(m, gx, gy)) return false;
        if (map_at_linear(m, gx, gy) < c.cr[k]) return false;
    }
    return true;
}

#endif  // PO_MAP_DEVICE_CODE

}  // namespace po
