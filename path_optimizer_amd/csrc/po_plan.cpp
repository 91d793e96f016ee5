// po_plan.cpp — PathOptimizer::solve for a batch of planning instances: the orchestration of the device stages
// (/root/reference/src/path_optimizer/path_optimizer.cpp:40-85,119-230 and ReferencePathSmoother::solve,
// src/reference_path_smoother/reference_path_smoother.cpp:34-48), plus the device-pointer entries of the small glue stages.
// Everything here goes through the public C ABI of the other stages; intermediates live in one arena of the handle.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <vector>

#include "../../include/po_hip.h"
#include "po_handle.hpp"
#include "po_launch.hpp"
#include "po_map.hpp"

extern "C" {

int po_bspline_batch_device(po_handle h, int B, int W, const int *n_way, const double *way_x, const double *way_y, int M, double *x, double *y, double *s, int *n_samples) {
    if (!h || B < 0 || W < 1 || M < 2 || (B > 0 && (!way_x || !way_y || !x || !y || !s || !n_samples))) return PO_ERR_INVALID;
    if (B == 0) return PO_OK;
    if (sizeof(double) * 2 * (size_t)W > 64 * 1024) return PO_ERR_UNSUPPORTED;
    Lock g(h->mu);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(po_launch_bspline(B, W, n_way, way_x, way_y, M, x, y, s, n_samples, h->stream));
    return PO_OK;
}

int po_segment_raw_batch_device(po_handle h, const po_spline_in *raw, int P, double *x, double *y, double *s, double *angle, double *k, int *n_points) {
    if (!h || P < 1 || !spline_args_ok(raw, false) || (raw->B > 0 && (!x || !y || !s || !angle || !k || !n_points))) return PO_ERR_INVALID;
    if (po_spline_lds_bytes(raw->K) > 64 * 1024) return PO_ERR_UNSUPPORTED;
    if (raw->B == 0) return PO_OK;
    const po::DevSpline D = make_dev_spline(raw);
    Lock g(h->mu);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(po_launch_segment_raw(&D, P, x, y, s, angle, k, n_points, h->stream));
    return PO_OK;
}

int po_post_project_batch_device(po_handle h, const po_spline_in *spline, int L, const int *n_layers, const double *layer_s, const double *offsets, double *x, double *y,
                                 double *s, double *length) {
    if (!h || L < 1 || !spline_args_ok(spline, false) || (spline->B > 0 && (!layer_s || !offsets || !x || !y || !s))) return PO_ERR_INVALID;
    if (po_spline_lds_bytes(spline->K) > 64 * 1024) return PO_ERR_UNSUPPORTED;
    if (spline->B == 0) return PO_OK;
    const po::DevSpline D = make_dev_spline(spline);
    Lock g(h->mu);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(po_launch_post_project(&D, L, n_layers, layer_s, offsets, x, y, s, length, h->stream));
    return PO_OK;
}

int po_segment_init_batch_device(po_handle h, const po_spline_in *spline, const double *start, int start_stride, const double *goal, int goal_stride, double *init, int *ok) {
    if (!h || start_stride < 3 || goal_stride < 2 || !spline_args_ok(spline) || (spline->B > 0 && (!start || !goal || !init || !ok))) return PO_ERR_INVALID;
    if (po_spline_lds_bytes(spline->K) > 64 * 1024) return PO_ERR_UNSUPPORTED;
    if (spline->B == 0) return PO_OK;
    const po::DevSpline D = make_dev_spline(spline);
    Lock g(h->mu);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(po_launch_segment_init(&D, start, start_stride, goal, goal_stride, h->params.enable_exact_position, init, ok, h->stream));
    return PO_OK;
}

// The argument check of po_plan_batch and po_plan_batch_device
static bool plan_args_ok(po_handle h, const po_plan_in *in, const po_plan_out *out) {
    if (!h || !in || !out || in->B < 0 || in->W < 4 || in->N < 2) return false;
    return in->B == 0 || (in->way_x && in->way_y && in->start && in->goal && out->states && out->n_states && out->ok);
}

// Layer capacity of the chain.  What the search may fill is the stride of postSmooth's QP, and that QP has to fit the on-chip tile: a capacity whose QP does not fit
// made po_smooth_batch_device refuse the whole batch (at search_long_spacing = 0.5 from max_length = 213 m on; never at the default 1.5, whose capacities stay below
// 370).  The footprint is not monotone in the size (chunk padding: 440 does not fit, 473 does), so: the smallest capacity >= want that fits, else the largest below
// it.  An instance that needs more layers than that comes back from the search with -2, i.e. stage 9, and the others are unaffected.
static int plan_layer_capacity(int want) {
    const size_t tile = 160 * 1024;
    want = std::min(want, 512);  // kDpMaxLayers of the search itself
    for (int L = want; L <= 512; ++L) if (po_smooth_lds_bytes(PO_SMOOTH_POST, L) <= tile) return L;
    for (int L = want - 1; L >= 4; --L) if (po_smooth_lds_bytes(PO_SMOOTH_POST, L) <= tile) return L;
    return want;
}

// The orchestration, under the call lock (the arena).  It cannot hold mu across the stage entries it calls (they take it themselves): what it needs of the handle's
// guarded state is read in one short section at the top, and its own launches go to that copy of the stream.
static int plan_device_locked(po_handle h, const po_plan_in *in, const po_plan_out *out) PO_REQUIRES(h->call_mu) {
    if (!plan_args_ok(h, in, out)) return PO_ERR_INVALID;
    if (!(in->max_length > 0)) return PO_ERR_INVALID;  // the device entry cannot look at the waypoints
    const int B = in->B;
    hipStream_t st;
    {
        Lock g(h->mu);
        if (!h->maps.d) return PO_ERR_INVALID;
        if (!assignment_covers(h, B)) return PO_ERR_INVALID;  // every instance needs its entry of the map assignment: refused before any stage is enqueued
        st = h->stream;
    }
    if (B == 0) return PO_OK;
    const po_params *prm = &h->params;
    HIP_TRY(hipSetDevice(h->device));
    // capacities from the waypoint polyline length: a B-spline is never longer than its control polygon
    const double Lmax = in->max_length;
    const int M = (int)std::ceil(Lmax) + 6, P = (int)std::ceil(Lmax) + 6;
    if (!(prm->search_long_spacing > 0)) return PO_ERR_UNSUPPORTED;  // (what the search stage would answer; here it would size Lc)
    const int Lc = plan_layer_capacity(std::max((int)std::ceil(std::min((Lmax + 3) / prm->search_long_spacing, 1e6)), 14) + 8);  // layers every search_long_spacing (0.5 m when <= 6 m long)
    const int N = in->N;
    const size_t bM = (size_t)B * M, bP = (size_t)B * P, bL = (size_t)B * Lc, bN = (size_t)B * N;
    const bool raw_out = prm->enable_raw_output != 0;
    // every intermediate is a slot of the handle's plan arena: declared here, sized from the declarations, resolved when the arena is reserved
    Stage A;
    auto D = [&A](size_t n) { return A.scratch<double>(n); };
    auto I = [&A](size_t n) { return A.scratch<int>(n); };
    auto Q = [&A](size_t n) { return A.scratch<po_info>(n); };
    const size_t nB = B;
    Slot<double> bs_x = D(bM), bs_y = D(bM), bs_s = D(bM);
    Slot<double> rw_x = D(bP), rw_y = D(bP), rw_s = D(bP), rw_a = D(bP), rw_k = D(bP);
    Slot<double> t2_x = D(bP), t2_y = D(bP), t2_s = D(bP);
    Slot<double> ly_s = D(bL), ly_lb = D(bL), ly_ub = D(bL), ly_off = D(bL);
    Slot<double> k2_x = D(bL), k2_y = D(bL), k2_s = D(bL);
    Slot<double> rf_x = D(bN), rf_y = D(bN), rf_z = D(bN), rf_k = D(bN), rf_s = D(bN);
    Slot<double> bnd = D(8 * bN);
    Slot<double> len1 = D(nB), len2 = D(nB), len3 = D(nB), l0 = D(nB), start3 = D(3 * nB);
    Slot<double> init = D(3 * nB), x0 = D(3 * nB), goal_z = D(nB);
    Slot<po_info> info1 = Q(nB), info2 = Q(nB), own_info3 = out->info ? Slot<po_info>{} : Q(nB);
    Slot<int> n_bs = I(nB), n_raw = I(nB), n_lay = I(nB), n_ref = I(nB), n_val = I(nB), okseg = I(nB);
    Slot<int> keep = I(nB), own_stage = out->stage ? Slot<int>{} : I(nB), gidx = I(nB), g_n = I(nB);
    // group staging + KPC limits (worst case: one group of everything)
    Slot<double> g_x = D(bN), g_y = D(bN), g_z = D(bN), g_k = D(bN), g_s = D(bN);
    Slot<double> g_b = D(8 * bN), g_x0 = D(3 * nB), g_goal = D(nB), g_states = D(5 * bN);
    Slot<po_info> g_info = Q(nB);
    Slot<double> lim_k = D(bN), lim_kp = D(bN);
    Slot<double> own_states = raw_out ? Slot<double>{} : D(5 * bN);  // QP states before the densifying output branch
    {
        Lock g(h->mu);
        PO_TRY(A.reserve(h, h->plan_arena));
    }
    po_info *info3 = out->info ? out->info : own_info3.ptr();
    int *stage = out->stage ? out->stage : own_stage.ptr();
    double *qp_states = raw_out ? out->states : own_states.ptr();  // optimizePath's two output branches (path_optimizer.cpp:191 / :201)

    po::PlanGate G{};
    G.B = B; G.stage = stage; G.start = in->start; G.goal = in->goal;
    G.mode = 0; G.start3 = start3;
    HIP_TRY(po_launch_plan_gate(&G, st));
    // 1. bSpline, 2. segmentRawReference
    PO_TRY(po_bspline_batch_device(h, B, in->W, in->n_way, in->way_x, in->way_y, M, bs_x, bs_y, bs_s, n_bs));
    po_spline_in raw{B, M, bs_s, bs_x, bs_y, n_bs, nullptr};
    PO_TRY(po_segment_raw_batch_device(h, &raw, P, rw_x, rw_y, rw_s, rw_a, rw_k, n_raw));
    // 3. TensionSmoother2::osqpSmooth
    const int smoother = prm->smoothing_method == PO_SMOOTH_TENSION ? PO_SMOOTH_TENSION : PO_SMOOTH_TENSION2;  // ReferencePathSmoother::create
    po_smooth_in s1{smoother, B, P, n_raw, rw_x, rw_y, rw_a, rw_k, rw_s, nullptr, nullptr, nullptr};
    po_smooth_out o1{t2_x, t2_y, t2_s, info1, nullptr};
    PO_TRY(po_smooth_batch_device(h, &s1, &o1));
    G.mode = 1; G.cnt = n_raw; G.cnt2 = n_bs; G.info = info1; G.s = t2_s; G.stride = P; G.length = len1;
    HIP_TRY(po_launch_plan_gate(&G, st));
    // 4. graphSearchDp on the smoothed spline (knots = the result lists, max_s = result_s.back() + 3)
    po_spline_in sp1{B, P, t2_s, t2_x, t2_y, n_raw, len1};
    PO_TRY(po_dp_search_batch_device(h, &sp1, start3, Lc, ly_s, ly_lb, ly_ub, l0, n_lay));
    G.mode = 2; G.cnt = n_lay;
    HIP_TRY(po_launch_plan_gate(&G, st));
    // 5. postSmooth: QP, then the re-projection -> second spline
    po_smooth_in s2{PO_SMOOTH_POST, B, Lc, n_lay, nullptr, nullptr, nullptr, nullptr, ly_s, ly_lb, ly_ub, l0};
    po_smooth_out o2{ly_off, nullptr, nullptr, info2, nullptr};
    PO_TRY(po_smooth_batch_device(h, &s2, &o2));
    G.mode = 3; G.info = info2;
    HIP_TRY(po_launch_plan_gate(&G, st));
    PO_TRY(po_post_project_batch_device(h, &sp1, Lc, n_lay, ly_s, ly_off, k2_x, k2_y, k2_s, len2));
    // 6. segmentSmoothedPath: initial errors, goal trim, re-sampling, corridor bounds
    po_spline_in sp2{B, Lc, k2_s, k2_x, k2_y, n_lay, len2};
    PO_TRY(po_segment_init_batch_device(h, &sp2, in->start, 4, in->goal, 3, init, okseg));
    G.mode = 4; G.init = init; G.ok = okseg; G.length = len3;
    HIP_TRY(po_launch_plan_gate(&G, st));
    po_spline_in sp3{B, Lc, k2_s, k2_x, k2_y, n_lay, len3};
    // path_optimizer.cpp:171-172: 0.15 / FLAGS_output_spacing when the QP states are output directly, 0.5 / 1.0 when they are densified later
    PO_TRY(po_resample_batch_device(h, &sp3, raw_out ? 0.15 : 0.5, raw_out ? prm->output_spacing : 1.0, N, rf_x, rf_y, rf_z, rf_k, rf_s, n_ref));
    po_bounds_in bi{B, N, Lc, rf_x, rf_y, rf_z, rf_s, n_ref, k2_s, k2_x, k2_y, n_lay};
    PO_TRY(po_bounds_batch_device(h, &bi, bnd, n_val));
    G.mode = 5; G.cnt = n_val; G.ref_s = rf_s; G.ref_stride = N; G.x0 = x0; G.goal_z = goal_z; G.keep = keep;
    HIP_TRY(po_launch_plan_gate(&G, st));
    // 7. the path QP, grouped by keep_control_steps_ (one launch = one keep)
    std::vector<int> h_stage(B), h_keep(B), h_nval(B), h_nref(B);
    HIP_TRY(hipMemcpyAsync(h_stage.data(), stage, sizeof(int) * B, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_keep.data(), keep, sizeof(int) * B, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_nval.data(), n_val, sizeof(int) * B, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_nref.data(), n_ref, sizeof(int) * B, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int form = prm->optimization_method == PO_K ? PO_K : (prm->optimization_method == PO_KPC ? PO_KPC : PO_KP);
    std::map<int, std::vector<int>> groups;
    bool capacity = false;
    for (int b = 0; b < B; ++b) {
        if (h_nref[b] == -2 && h_stage[b] == 6) { h_stage[b] = 9; capacity = true; }  // N too small for the re-sampled reference
        if (h_stage[b] == 0) groups[form == PO_KP ? h_keep[b] : (form == PO_KPC ? 4 : 1)].push_back(b);  // K has no held control, KPC fixes keep = 4
    }
    if (form == PO_KPC) {
        std::vector<double> hk((size_t)bN, std::tan(prm->max_steer) / prm->wheel_base), hkp((size_t)bN, 1.7976931348623157e308);
        HIP_TRY(hipMemcpyAsync(lim_k, hk.data(), sizeof(double) * bN, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(lim_kp, hkp.data(), sizeof(double) * bN, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    for (auto &kv : groups) {
        const std::vector<int> &ids = kv.second;
        const int Gn = (int)ids.size();
        int Ng = 2;
        for (int b : ids) Ng = std::max(Ng, h_nval[b]);
        HIP_TRY(hipMemcpyAsync(gidx, ids.data(), sizeof(int) * Gn, hipMemcpyHostToDevice, st));
        po::PlanRows R{};
        R.G = Gn; R.N = N; R.Ng = Ng; R.idx = gidx;
        R.ref_x = rf_x; R.ref_y = rf_y; R.ref_z = rf_z; R.ref_k = rf_k; R.ref_s = rf_s; R.bounds = bnd; R.x0 = x0; R.goal_z = goal_z; R.n_valid = n_val;
        R.g_x = g_x; R.g_y = g_y; R.g_z = g_z; R.g_k = g_k; R.g_s = g_s; R.g_bounds = g_b; R.g_x0 = g_x0; R.g_goal = g_goal; R.g_n = g_n;
        R.g_states = g_states; R.g_info = g_info; R.states = qp_states; R.info = info3;
        HIP_TRY(po_launch_plan_gather(&R, st));
        // KPC with a spline-built reference: updateLimits() has no speed profile ("Reference states must be given directly!") and falls back to
        // max_k = tan(max_steering_angle) / wheel_base, max_kp = DBL_MAX (reference_path_impl.cpp:214-222)
        const double *gk = form == PO_KPC ? lim_k.ptr() : nullptr, *gkp = form == PO_KPC ? lim_kp.ptr() : nullptr;
        po_batch_in qi{form, Gn, Ng, kv.first, g_x, g_y, g_z, g_k, g_s, g_b, g_x0, g_goal, gk, gkp, g_n};
        po_batch_out qo{g_states, g_info, nullptr};
        const int rc = po_solve_batch_device(h, &qi, &qo);
        if (rc == PO_ERR_UNSUPPORTED) {  // does not fit the on-chip tile: flagged per instance, the others go on
            for (int b : ids) h_stage[b] = 9;
            capacity = true;
            HIP_TRY(hipStreamSynchronize(st));  // gidx is reused by the next group
            continue;
        }
        PO_TRY(rc);
        HIP_TRY(po_launch_plan_scatter(&R, st));
        HIP_TRY(hipStreamSynchronize(st));  // gidx / staging are reused by the next group
    }
    if (capacity) HIP_TRY(hipMemcpyAsync(stage, h_stage.data(), sizeof(int) * B, hipMemcpyHostToDevice, st));
    HIP_TRY(po_launch_plan_clear(B, N, stage, qp_states, info3, st));
    G.mode = 6; G.cnt = n_val; G.info = info3;
    HIP_TRY(po_launch_plan_gate(&G, st));
    // 8. the tail of optimizePath: arc length + collision check + truncation rule
    if (raw_out) PO_TRY(po_postcheck_batch_device(h, B, N, n_val, out->states, info3, out->n_states, out->ok));
    else PO_TRY(po_densify_batch_device(h, B, N, n_val, qp_states, info3, N, out->states, out->n_states, out->ok));
    G.mode = 7; G.cnt = out->n_states; G.ok = out->ok;
    HIP_TRY(po_launch_plan_gate(&G, st));
    return PO_OK;
}

int po_plan_batch_device(po_handle h, const po_plan_in *in, const po_plan_out *out) {
    if (!h) return PO_ERR_INVALID;
    Lock call(h->call_mu);
    return plan_device_locked(h, in, out);
}

int po_plan_batch(po_handle h, const po_plan_in *in, const po_plan_out *out) {
    if (!plan_args_ok(h, in, out)) return PO_ERR_INVALID;
    const int B = in->B;
    if (B == 0) return PO_OK;
    double Lmax = in->max_length;
    if (!(Lmax > 0)) {
        Lmax = 1.0;
        for (int b = 0; b < B; ++b) {
            const int n = in->n_way ? in->n_way[b] : in->W;
            double len = 0;
            for (int i = 0; i + 1 < n && i + 1 < in->W; ++i) len += std::hypot(in->way_x[(size_t)b * in->W + i + 1] - in->way_x[(size_t)b * in->W + i], in->way_y[(size_t)b * in->W + i + 1] - in->way_y[(size_t)b * in->W + i]);
            Lmax = std::max(Lmax, len);
        }
    }
    HIP_TRY(hipSetDevice(h->device));
    const size_t nB = B, bw = nB * in->W;
    Stage S;  // the staging block of the host-pointer entry (the arena belongs to the device entry)
    const Slot<double> wx = S.in(in->way_x, bw), wy = S.in(in->way_y, bw), d_start = S.in(in->start, 4 * nB), d_goal = S.in(in->goal, 3 * nB);
    const Slot<int> d_nway = S.in(in->n_way, nB);
    // stage / info: the device arrays always exist and the stages write them; a null host pointer only skips the copy back
    const Slot<double> d_states = S.out(out->states, nB * in->N * 5);
    const Slot<int> d_n = S.out(out->n_states, nB), d_ok = S.out(out->ok, nB), d_stage = S.out(out->stage, nB);
    const Slot<po_info> d_info = S.out(out->info, nB);
    // the sequence of staged_call (po_handle.hpp), written out: the twin needs the call lock this function holds, and a callable cannot state that
    Lock call(h->call_mu);
    {
        Lock g(h->mu);
        PO_TRY(S.upload(h, h->plan_host));
    }
    po_plan_in din = *in;
    din.way_x = wx; din.way_y = wy; din.start = d_start; din.goal = d_goal; din.n_way = d_nway; din.max_length = Lmax;
    const po_plan_out dout{d_states, d_n, d_ok, d_stage, d_info};
    PO_TRY(plan_device_locked(h, &din, &dout));
    Lock g(h->mu);
    return S.copy_out(h);
}

}  // extern "C"
