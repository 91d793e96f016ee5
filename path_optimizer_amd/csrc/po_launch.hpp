// po_launch.hpp — every internal entry of libpo_hip.so that one translation unit defines and another calls, declared ONCE.  These functions have C linkage: no
// name mangling, so a prototype that drifts from its definition would link and pass garbage.  Both sides include this header — the file that defines an entry and
// every file that calls it — which turns such a drift into a compile error (conflicting declaration).  A new entry gets its prototype here and nowhere else.
// Declarations only (forward-declared structs): po_edt.hip, po_raster.hip and po_scene.hip, which share no header with the solve kernels, include it too.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/po_hip.h"

namespace po {
struct DevBatch; struct DevParams;                                                   // po_device.hpp
struct Shape;                                                                        // po_solve_common.hpp
// what an object of the solve kernels holds: the uniform-row-class / general variant of the solve kernels (the general object: also the polish kernels), the Newton
// kernels (both phases and the fallback), or the length-specialised uniform warm start / first / second Newton launch / the two Newton launches with the standard row
// classes as compile-time constants
enum { kObjUni, kObjGen, kObjNewton, kObjFixUni, kObjFixNewton1, kObjFixNewton2, kObjFixNewtonStd1, kObjFixNewtonStd2 };
// what an entry is asked to launch (Newton: phase 1 or 2 by DevBatch::nw_phase; NewtonStd: the constant-class kernel of a fixed length; StdSelect: the kernel that
// decides which paths that kernel gets)
enum { kLaunchSolve, kLaunchNewton, kLaunchFallback, kLaunchPolish, kLaunchNewtonStd, kLaunchStdSelect };
// the groups the shapes are dealt to the objects in (KP's two-level shapes: one lane per chunk / role-split / multi-group / the wide role-split shapes by SPL; the single-level mapping)
enum { kGrpLane = 1, kGrpSplit = 2, kGrpMulti = 4, kGrpW56 = 8, kGrpW7 = 16, kGrpW8 = 32, kGrpOne = 64 };
// Everything the host asks about the shape of a batch (formulation, N, C, keep), filled ONCE per call by po_resolve_solve and handed to the launches.  A plain struct
// of host-side answers: no kernel sees it.
struct SolveShape {
    int nt, spl, two, nwx;            // the Shape of po_solve_common.hpp (nt == 0: no shape holds the batch)
    size_t lds;                       // dynamic LDS bytes of its kernels (no shape: 1 GB; may exceed the 160 KB a launch can have: the entries refuse that)
    int group;                        // the group of the table row that equals the shape (0: none)
    int uni, polish, fixed;           // a uniform-row-class variant exists / a polish kernel exists / a length-specialised instantiation exists for this length
    int state_doubles, park_doubles;  // doubles per path of the state block and of a parked Newton path's block (0: the single-level mapping)
};
constexpr size_t kLdsLimit = 160 * 1024;
struct DevMap; struct DevMaps; struct DevCar; struct DevBounds; struct DevSpline; struct DevSearch;  // po_map.hpp
struct DevResample; struct PlanGate; struct PlanRows; struct DevSelect; struct DevSpeed; struct DevDynamic; struct DevStplan; struct DevNudge;
struct DevTrajectory; struct DevAgentSets; struct DevStgo; struct DevSpeedQp;
struct DevSmooth;                                                                    // po_smooth.hpp
}  // namespace po

extern "C" {
// ---- po_kernels.hip: the solve, by formulation ----
// the shape of a batch, resolved: 1 and *s filled, or 0 when no shape holds it (*s zeroed, lds = 1 GB).  The four launches take what it filled and resolve nothing.
int po_resolve_solve(int form, int N, int C, int keep, po::SolveShape *s);
hipError_t po_launch_solve(int form, const po::SolveShape *s, const po::DevBatch *in, const po::DevParams *P, hipStream_t st);
hipError_t po_launch_newton(int form, const po::SolveShape *s, const po::DevBatch *in, const po::DevParams *P, hipStream_t st);
hipError_t po_launch_newton_std(int form, const po::SolveShape *s, const po::DevBatch *in, const po::DevParams *P, hipStream_t st);
hipError_t po_launch_newton_fallback(int form, const po::SolveShape *s, const po::DevBatch *in, const po::DevParams *P, hipStream_t st);
hipError_t po_launch_polish(int form, const po::SolveShape *s, const po::DevBatch *in, const po::DevParams *P, hipStream_t st);
hipError_t po_launch_finalize_status(po_info *info, int B, hipStream_t st);
hipError_t po_launch_mark_unavailable(po_info *info, int B, int refine, int polish, hipStream_t st);
hipError_t po_launch_nw_sort(const int *keys, int B, int *list, const int *flag, int *list2, hipStream_t st);
hipError_t po_launch_scale(int form, const po::DevBatch *in, const po::DevParams *P, int passes, double *sc, int *nw_keys, int *fb_count, int *std_block, hipStream_t st);
hipError_t po_launch_assemble(int form, const po::DevBatch *in, const po::DevParams *P, double *l, double *u, double *dyn, hipStream_t st);
size_t po_lds_bytes(int form, int N, int C, int keep);
int po_shape_threads(int form, int N, int C, int keep);
int po_polish_state_doubles(int form, int N, int C, int keep);
int po_newton_park_doubles(int form, int N, int C, int keep);
int po_has_polish_kernel(int form, int N, int C, int keep);
int po_has_fixed_length(int form, int N, int C, int keep);

// ---- po_solve.cpp: what a solve of B paths of this shape will launch (plan_solve: no HIP call, no handle), exported for tests/test_solve_plan.py like the queries above.
// out[9]: split, state block, polish, sliced, fixed, the refine mark, the polish mark, count read back, warm-start decades (its eps is 10^that times the caller's)
int po_plan_solve(int form, int N, int keep, int B, int ragged, int refine, int refine_rounds, int refine_extra_rounds, int refine_chain, int polish, int nw_slice,
                  int slice_forced, int fixed_on, int wave_slots, int *out);

// ---- po_solve_form.hip: the objects that hold the solve kernels.  X(object, formulation, kind, shape groups it holds): ONE entry per object, named like the object (the
// Makefile compiles <object>.o with -DPO_ENTRY=<object>), one signature for all.  The object reads its own row here; the dispatcher (po_kernels.hip) builds its route
// table from the same list, and the link fails on an object the Makefile's list lacks.  The groups are those of po_solve_common.hpp's table of shapes.
#define PO_SOLVE_OBJECTS(X)                                                     \
    X(po_solve_kp_uni, F_KP, kObjUni, kGrpLane | kGrpSplit | kGrpMulti)         \
    X(po_solve_kp, F_KP, kObjGen, kGrpLane | kGrpSplit | kGrpMulti | kGrpOne)   \
    X(po_solve_kp_w_uni, F_KP, kObjUni, kGrpW56 | kGrpW7 | kGrpW8)              \
    X(po_solve_kp_w, F_KP, kObjGen, kGrpW56 | kGrpW7 | kGrpW8)                  \
    X(po_solve_kpc_uni, F_KPC, kObjUni, kGrpLane)                               \
    X(po_solve_kpc, F_KPC, kObjGen, kGrpLane | kGrpOne)                         \
    X(po_solve_k_uni, F_K, kObjUni, kGrpLane)                                   \
    X(po_solve_k, F_K, kObjGen, kGrpLane | kGrpOne)                             \
    X(po_newton_kp, F_KP, kObjNewton, kGrpLane)                                 \
    X(po_newton_kp_b, F_KP, kObjNewton, kGrpSplit)                              \
    X(po_newton_kp_c, F_KP, kObjNewton, kGrpMulti)                              \
    X(po_newton_kp_w1, F_KP, kObjNewton, kGrpW56)                               \
    X(po_newton_kp_w2, F_KP, kObjNewton, kGrpW7)                                \
    X(po_newton_kp_w3, F_KP, kObjNewton, kGrpW8)                                \
    X(po_newton_kpc, F_KPC, kObjNewton, kGrpLane)                               \
    X(po_newton_k, F_K, kObjNewton, kGrpLane)                                   \
    X(po_solve_kp_fix_uni, F_KP, kObjFixUni, kGrpLane)                          \
    X(po_newton_kp_fix1, F_KP, kObjFixNewton1, kGrpLane)                        \
    X(po_newton_kp_fix2, F_KP, kObjFixNewton2, kGrpLane)                        \
    X(po_newton_kp_fixstd1, F_KP, kObjFixNewtonStd1, kGrpLane)                  \
    X(po_newton_kp_fixstd2, F_KP, kObjFixNewtonStd2, kGrpLane)
#if defined(PO_DEV_HEADLINE) && !defined(PO_ENTRY)  // `make dev` links three of the KP objects: the dispatcher built for it answers hipErrorNotSupported for the others
#define PO_OBJECT_ATTR __attribute__((weak))
#else
#define PO_OBJECT_ATTR
#endif
#define PO_X(name, form, kind, groups) \
    PO_OBJECT_ATTR hipError_t name(int launch, const po::Shape &s, size_t lds, const po::DevBatch *in, const po::DevParams *P, hipStream_t st);
PO_SOLVE_OBJECTS(PO_X)
#undef PO_X

// ---- po_post.hip: map stages, spline stages, the glue of po_plan ----
hipError_t po_launch_postcheck(const po::DevMaps *m, const po::DevCar *c, int B, int N, const int *n_points, const double *states, const po_info *info, int *n_valid,
                               int *ok, hipStream_t st);
hipError_t po_launch_densify(const po::DevMaps *m, const po::DevCar *c, int B, int N, const int *n_points, const double *states, const po_info *info, double spacing,
                             int M, double *out, int *n_out, int *ok, hipStream_t st);
hipError_t po_launch_map_sample(const po::DevMaps *m, int layer, int n, const double *xy, double *dist, int *inside, hipStream_t st);
hipError_t po_launch_bounds(const po::DevMaps *m, const po::DevBounds *in, double *bounds, int *n_valid, hipStream_t st);
hipError_t po_launch_resample(const po::DevSpline *in, const po::DevResample *r, hipStream_t st);
hipError_t po_launch_limits(int B, int N, const int *n_points, const double *v, const double *a, double *max_k, double *max_kp, double mu, double rate, hipStream_t st);
hipError_t po_launch_dp_search(const po::DevMaps *m, const po::DevSpline *in, const po::DevSearch *q, int one_wave, int *waves_used, hipStream_t st);  // *waves_used: 8 or 1
size_t po_dp_lds_bytes(int K, int L);
size_t po_spline_lds_bytes(int K);
hipError_t po_launch_bspline(int B, int W, const int *n_way, const double *wx, const double *wy, int M, double *x, double *y, double *s, int *n_samples, hipStream_t st);
hipError_t po_launch_segment_raw(const po::DevSpline *in, int P, double *x, double *y, double *s, double *angle, double *k, int *n_points, hipStream_t st);
hipError_t po_launch_post_project(const po::DevSpline *in, int L, const int *n_layers, const double *layer_s, const double *off, double *x, double *y, double *s,
                                  double *length_out, hipStream_t st);
hipError_t po_launch_segment_init(const po::DevSpline *in, const double *start, int start_stride, const double *goal, int goal_stride, int exact, double *init, int *ok,
                                  hipStream_t st);
hipError_t po_launch_plan_gate(const po::PlanGate *g, hipStream_t st);
hipError_t po_launch_plan_gather(const po::PlanRows *r, hipStream_t st);
hipError_t po_launch_plan_scatter(const po::PlanRows *r, hipStream_t st);
hipError_t po_launch_plan_clear(int B, int N, const int *stage, double *states, po_info *info, hipStream_t st);

// ---- po_smooth.hip: the reference-smoothing QPs ----
hipError_t po_launch_smooth(const po::DevSmooth *a, int *variant_used, hipStream_t st);  // *variant_used: 100 * kind + 10 * waves per QP + WPE of the instantiation launched
size_t po_smooth_lds_bytes(int kind, int P);
size_t po_smooth_scratch_doubles(int kind, int P);
int po_smooth_blocked(int kind, int P);

// ---- po_edt.hip: occupancy image -> distance layer ----
hipError_t po_launch_edt(const unsigned char *cells, int M, int sx, int sy, float res, void *scratch, float *out, hipStream_t st);
size_t po_edt_scratch_bytes(int M, int sx, int sy);
int po_edt_max_side(void);
int po_edt_max_images(void);

// ---- po_raster.hip: per-layer obstacle lists -> occupancy images (every pointer, those inside *lists too, is a device pointer) ----
hipError_t po_launch_raster(const po_obstacle_lists *lists, int M, const double *pos_xy, unsigned char *out, hipStream_t st);

// ---- po_scene.hip: the world grid and the rings of *scene ORed into po_launch_raster's image of scene->lists (device pointers; world == nullptr: no world clause) ----
hipError_t po_launch_scene(const po_scene *scene, int M, const double *pos_xy, const po_occupancy *world, int outside_occupied, unsigned char *img, hipStream_t st);

// ---- po_select.hip: score and select (the clamped group table into a->gs, then one wave per candidate, then one wave per group; device pointers) ----
hipError_t po_launch_select(const po::DevMaps *m, const po::DevCar *c, const po::DevSelect *a, hipStream_t st);

// ---- po_speed.hip: the speed profile (caps: one wave per path; then the three sweeps: one lane per path, 64 paths per workgroup; device pointers) ----
hipError_t po_launch_speed(const po::DevMaps *m, const po::DevCar *c, const po::DevSpeed *a, hipStream_t st);

// ---- po_dynamic.hip: timed paths against moving agents (one wave per path, lanes over intervals, the path's agent set through LDS in chunks; device pointers) ----
hipError_t po_launch_dynamic(const po::DevCar *c, const po::DevDynamic *a, hipStream_t st);

// ---- po_stplan.hip: station-time speed planning (one workgroup per path: blocked cells over the lanes with the agent set through LDS in chunks, then the layered
// search in LDS; dynamic LDS sized from K, a->Mb and U; device pointers) ----
hipError_t po_launch_stplan(const po::DevCar *c, const po::DevStplan *a, hipStream_t st);

// ---- po_stgo.hip: station-time plans that resume, sampled in time (one workgroup per path: the phases of po_stplan.hip's search from po_stsearch.hpp with a stopped
// predecessor free to pull away, then lanes over the Q samples, each with a binary search on the path's s row; the same dynamic LDS; device pointers) ----
hipError_t po_launch_stgo(const po::DevCar *c, const po::DevStgo *a, hipStream_t st);

// ---- po_speedqp.hip: the speed QP inside a plan's tunnel (one wave per path: lanes over samples and rows for the row operations, lane 0 for the banded
// factorisation and the two substitutions; dynamic LDS sized from Q; device pointers) ----
hipError_t po_launch_speedqp(const po::DevSpeedQp *a, hipStream_t st);

// ---- po_nudge.hip: corridor nudge (one wave per path, lanes own fixed (state, circle) pairs of the corridor, which lives in the output; the path's agent set through
// LDS in chunks; device pointers) ----
hipError_t po_launch_nudge(const po::DevNudge *a, hipStream_t st);

// ---- po_trajectory.hip: timed trajectory (one wave per path: a validity sweep over the rows, then lanes over the samples, each with a binary search on the path's
// t row; the agent records by the first lanes; no LDS; device pointers) ----
hipError_t po_launch_trajectory(const po::DevTrajectory *a, hipStream_t st);

// ---- po_agentsets.hip: agent sets (count: one wave per ego, lanes over the rows, then over the candidates 64 at a time; scan: one workgroup over count; gather:
// one wave per ego, the same decisions, the kept records copied by the whole wave; skipped when capacity is 0; 256 bytes of LDS; device pointers) ----
hipError_t po_launch_agentsets(const po::DevAgentSets *a, hipStream_t st);
}  // extern "C"
