// po_solve.cpp — the solve entries of the C ABI (include/po_hip.h), the two diagnostics that share their argument check and the timing read-backs.  A solve resolves the
// shape of its batch ONCE (po_resolve_solve, po_kernels.hip), then takes four steps: plan_solve decides what will be launched (no HIP call: testable
// without a GPU), provision grows the handle's blocks, enqueue issues the launches and event records, dump_cycles is the developer read-back.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/po_hip.h"
#include "po_device.hpp"
#include "po_handle.hpp"
#include "po_launch.hpp"

namespace {
struct CopySeg { char *dst; const char *src; size_t bytes; };
// memcpy of a list of segments on `nthr` host threads (pieces of <= 2 MB handed out round-robin: every thread streams through every array)
void parallel_copy(const std::vector<CopySeg> &segs, int nthr) {
    std::vector<CopySeg> pieces;
    const size_t kPiece = (size_t)2 << 20;
    for (const CopySeg &sg : segs)
        for (size_t o = 0; o < sg.bytes; o += kPiece) pieces.push_back({sg.dst + o, sg.src + o, std::min(kPiece, sg.bytes - o)});
    if (nthr <= 1 || pieces.size() <= 1) {
        for (const CopySeg &pc : pieces) std::memcpy(pc.dst, pc.src, pc.bytes);
        return;
    }
    nthr = (int)std::min<size_t>((size_t)nthr, pieces.size());
    std::vector<std::thread> th;
    for (int t = 1; t < nthr; ++t)
        th.emplace_back([&pieces, t, nthr] { for (size_t i = (size_t)t; i < pieces.size(); i += (size_t)nthr) std::memcpy(pieces[i].dst, pieces[i].src, pieces[i].bytes); });
    for (size_t i = 0; i < pieces.size(); i += (size_t)nthr) std::memcpy(pieces[i].dst, pieces[i].src, pieces[i].bytes);
    for (std::thread &t : th) t.join();
}

po::DevParams make_dev_params(const po_params &p, int form, int keep) {
    po::DevParams D;
    D.d1 = p.d[0]; D.d2 = p.d[1]; D.d3 = p.d[2]; D.d4 = p.d[3];
    if (form == PO_K) {
        D.w_dev = p.k_w_dev; D.w_c = p.k_w_curv; D.w_cr = p.k_w_curv_rate; D.w_s1 = p.w_slack; D.w_s2 = 0; D.w_u = 0; D.w_su = 0;
    } else {
        D.w_dev = p.w_dev; D.w_c = p.w_curv; D.w_cr = p.w_curv_rate; D.w_s1 = p.w_slack;
        D.w_s2 = (form == PO_KPC) ? p.w_k_slack : 0.0;
        D.w_u = keep * p.w_curv_rate;
        D.w_su = (form == PO_KPC) ? p.w_kp_slack * keep : 0.0;
    }
    D.margin = p.margin;
    D.kmax = std::tan(p.max_steer) / p.wheel_base;
    D.max_steer = p.max_steer;
    D.wheel_base = p.wheel_base;
    D.sigma = p.sigma; D.alpha = p.alpha; D.rho0 = p.rho0; D.eps_abs = p.eps_abs; D.eps_rel = p.eps_rel;
    D.eps_pinf = p.eps_prim_inf; D.adapt_tol = p.adapt_tol;
    D.max_iter = p.max_iter; D.check_every = p.check_every; D.adapt_every = p.adapt_every;
    D.end_heading = p.constraint_end_heading;
    D.polish = p.polish; D.pol_delta = p.polish_delta > 0 ? p.polish_delta : 1e-6; D.pol_refine = p.polish_refine_iter < 0 ? 0 : p.polish_refine_iter;
    D.refine = p.refine; D.ref_eps = p.refine_eps; D.ref_rounds = p.refine_rounds;
    D.ref_extra = (p.refine && p.refine_extra_rounds > 0) ? p.refine_extra_rounds : 0;
    // every refine_newton_* field is defaulted when it is not positive (a zero-initialised po_params must not silently disable the penalty growth) and held inside what
    // the rest of the engine allows; the ESCALATED caps (refine_newton_escalate: up to 100 x) are clamped inside the phase to kRhoMax / 1e8 (po_fast.inc, oracle alike)
    D.ref_nw_rho = p.refine_newton_rho > 0 ? std::min(p.refine_newton_rho, po::kRhoMax) : 100.0;
    D.ref_nw_rho_eq = p.refine_newton_rho_eq > 0 ? std::min(p.refine_newton_rho_eq, 1e8) : 1e4;
    D.ref_nw_rho_max = p.refine_newton_rho_max > 0 ? std::min(p.refine_newton_rho_max, po::kRhoMax) : 1e5;
    D.ref_nw_rho_eq_max = p.refine_newton_rho_eq_max > 0 ? std::min(p.refine_newton_rho_eq_max, 1e8) : (p.refine_newton_rho_eq_max < 0 ? 1e6 : 0.0);  // 0: the equality penalty never grows (documented switch)
    D.ref_ls_tol = p.refine_ls_tol > 0 ? p.refine_ls_tol : 1e-4;
    D.ref_nw_final = p.refine_newton_final; D.ref_nw_esc = p.refine_newton_escalate; D.ref_nw_slice = 0; D.ref_ls_max = p.refine_ls_max > 0 ? p.refine_ls_max : 30; D.ref_nw_max = p.refine_newton_max > 0 ? p.refine_newton_max : 300;
    return D;
}

// the argument check of every entry here; on PO_OK the dimensions and the resolved shape of the batch: the one resolution of the call
struct Dims { int n, m, C; po::SolveShape shape; };
int validate(const po_batch_in *in, Dims *d) {
    if (!in || in->B < 0) return PO_ERR_INVALID;
    PO_TRY(po_problem_dims(in->formulation, in->N, in->keep, &d->n, &d->m, &d->C));
    if (!in->ref_x || !in->ref_y || !in->ref_z || !in->ref_k || !in->ref_s || !in->bounds || !in->x0 || !in->goal_z) return PO_ERR_INVALID;
    if (in->formulation == PO_KPC && (!in->max_k || !in->max_kp)) return PO_ERR_INVALID;
    po_resolve_solve(in->formulation, in->N, d->C, in->keep, &d->shape);
    return d->shape.lds > po::kLdsLimit ? PO_ERR_UNSUPPORTED : PO_OK;  // (no shape at all: 1 GB)
}

po::DevBatch fill_dev_batch(const po_handle_s *h, const po_batch_in *in, const po_batch_out *out, const Dims &d) PO_REQUIRES(h->mu) {
    po::DevBatch D{};  // (what a solve's launches are handed between them — state block, work lists, phase marks, dbg_cycles, fixed_len — starts as 0 / nullptr: the solve sets it)
    D.B = in->B; D.N = in->N; D.keep = in->keep; D.C = d.C;
    D.ref_x = in->ref_x; D.ref_y = in->ref_y; D.ref_z = in->ref_z; D.ref_k = in->ref_k; D.ref_s = in->ref_s;
    D.bounds = in->bounds; D.x0 = in->x0; D.goal_z = in->goal_z; D.max_k = in->max_k; D.max_kp = in->max_kp;
    D.n_points = in->n_points;
    D.order = in->order;
    D.out_states = out ? out->states : nullptr;
    D.out_info = out ? out->info : nullptr;
    D.out_x = out ? out->x : nullptr;
    if (!h->env_identity && in->B > 8)  // perm_bits, the block -> path permutation (0, po_debug_set "identity_order": blockIdx order, dev tool)
        while ((1 << D.perm_bits) < in->B) ++D.perm_bits;
    D.n = d.n; D.m = d.m;
    return D;
}

// ---- step 1: the schedule of a solve — what will be launched for B paths of this shape under these parameters.  A function of its arguments: no HIP call, no handle.
struct SolveSchedule {
    bool state;               // the solve kernels leave the ADMM state in pol_buf: OSQP's polish (opt-in) and the Newton refinement pick it up there
    bool split, sliced;       // refine = 2: plain warm-start launches, the Newton refinement as its own launch (sliced: as two, below), then the fallback launch for the later rounds
    bool polish, fixed;       // the polish launch follows / the length-specialised kernels run the batch
    bool std_classes;         // ... and their Newton launches are the constant-class pair, each followed by the kernel without the constants over what it left
    bool no_refine, no_polish;  // asked for, but this shape has no kernel for it: status_refine / status_polish = PO_NOT_AVAILABLE on every path instead of the "off" value 0
    bool read_back;           // the fallback launch is issued only when the count read back says that a path is on its list (refine_chain = 3: always issued, asynchronous)
    int warm_decades;         // the warm start stops where round 0 of the rounds stops: at 10^warm_decades x eps
};
SolveSchedule plan_solve(const po_params &p, const po::SolveShape &s, int B, bool ragged, int nw_slice, bool slice_forced, bool fixed_on, int wave_slots, bool classes_on) {
    SolveSchedule q{};
    const int rounds = p.refine_rounds > 1 ? p.refine_rounds : 1;
    const int rounds_total = rounds + ((p.refine && p.refine_extra_rounds > 0) ? p.refine_extra_rounds : 0);
    // (shapes on the single-level mapping have neither kernel, the role-split shapes of keep 6 .. 16 no polish kernel: the marks)
    q.state = (p.polish || p.refine) && s.state_doubles > 0;
    q.polish = p.polish && q.state && s.polish;
    q.split = p.refine == 2 && q.state && rounds_total < 32;
    // SLICED LAUNCHES (engine-internal scheduling): the Newton launch is two — every path for nw_slice steps, the unfinished ones parked with a
    // priority key; a one-workgroup sort; the parked paths in order of expected remaining work, longest first: one launch in engine order ends on a tail of a few long
    // paths.  Statuses and certificates do not depend on the slicing, solutions agree to round-off.  Left alone the engine slices where it was measured to pay: one wave
    // per path (NT = 64: 4 x CUs paths at a time) and at least two rounds of them (config 3 4.76 -> 4.06 ms; two-wave shapes and batches of one round gain nothing or lose).
    q.sliced = q.split && nw_slice > 0 && (slice_forced || (B >= 2 * wave_slots && s.nt == 64));
    q.fixed = fixed_on && !ragged && s.fixed;  // the switch is on, every path has the batch's length and the length is a listed one
    q.std_classes = q.fixed && q.split && classes_on;  // (a launch of the solve tests every path's classes: no property of the batch is asked here)
    q.no_refine = p.refine == 2 && !q.split;
    q.no_polish = p.polish && !q.polish;
    q.read_back = p.refine_chain != 3;
    q.warm_decades = rounds - 1;
    return q;
}

// ---- step 2: every block the schedule needs, grown on the handle.  The parking blocks of the sliced launches are 39 KB per path on top of the state block: a batch
// they do not fit beside is solved unsliced (*q says so) — scheduling is not worth an out-of-memory error.
int provision(po_handle h, const po::SolveShape &s, size_t B, SolveSchedule *q) PO_REQUIRES(h->mu) {
    if (h->env_cycles) PO_TRY(h->dbg_buf.ensure(sizeof(long long) * 16 * B));
    PO_TRY(h->scale_buf.ensure(sizeof(double) * 64 * B));
    if (q->state) PO_TRY(h->pol_buf.ensure(sizeof(double) * (size_t)s.state_doubles * B));
    h->std_B = 0; h->std_flag_at = h->std_left2_at = -1;  // (what the read-backs of po_debug_get look at: nothing yet from THIS solve)
    if (!q->split) return PO_OK;
    PO_TRY(h->fb_buf.ensure(sizeof(int) * (B + 1)));
    PO_TRY(h->fb_host.ensure(64));
    // (keys [B] and list [B + 1]; the constant-class kernels keep their lists behind them and need the block on an unsliced solve too — without it they are not run)
    const size_t idx_bytes = sizeof(int) * (q->std_classes ? po::std_lists_ints(B) : 2 * B + 1);
    if (q->sliced && (h->nw_state_buf.ensure(sizeof(double) * (size_t)s.park_doubles * B) || h->nw_idx_buf.ensure(idx_bytes))) {
        (void)hipGetLastError();
        h->nw_state_buf.release();
        q->sliced = false;
    }
    if (q->std_classes && h->nw_idx_buf.ensure(idx_bytes)) {
        (void)hipGetLastError();
        q->std_classes = false;
    }
    h->nw_last_B = q->sliced ? (int)B : 0;
    h->std_flag_at = q->std_classes ? (long)po::std_flag_index(B) : -1;
    h->std_B = q->std_classes ? (int)B : 0;
    h->std_left2_at = q->std_classes && q->sliced ? (long)po::std_left2_index(B) : -1;
    return PO_OK;
}

// ---- step 3: the launches and the event records of the schedule, on the handle's stream
int enqueue(po_handle h, int form, const po::SolveShape &s, const SolveSchedule &q, po::DevBatch &D, po::DevParams &P) PO_REQUIRES(h->mu) {
    const int B = D.B;
    if (h->env_cycles) {
        D.dbg_cycles = static_cast<long long *>(h->dbg_buf.p);
        HIP_TRY(hipMemsetAsync(D.dbg_cycles, 0, sizeof(long long) * 16 * (size_t)B, h->stream));
    }
    D.scale = static_cast<double *>(h->scale_buf.p);
    if (q.state) { D.pol_state = static_cast<double *>(h->pol_buf.p); D.pol_stride = s.state_doubles; }
    HIP_TRY(hipEventRecord(h->ev0, h->stream));
    h->timed_phases = false;
    // per-path equilibration (h->params.scaling class-level Ruiz passes; 0 -> identity), then the fused solve.  The same launch resets what the Newton launches count in:
    // the fall-back work list's count, and the park keys to -1 (a path no workgroup of the first sliced launch reaches — a malformed caller-side order — is not parked)
    // ... and the lists and the count of the constant-class Newton kernels
    int *const nw_block = static_cast<int *>(h->nw_idx_buf.p);
    HIP_TRY(po_launch_scale(form, &D, &P, h->params.scaling, static_cast<double *>(h->scale_buf.p), q.sliced ? nw_block : nullptr,
                            q.split ? static_cast<int *>(h->fb_buf.p) : nullptr, q.std_classes ? nw_block : nullptr, h->stream));
    if (q.split) {
        po::DevParams P1 = P;  // the warm start: the plain solve kernels, stopped where round 0 of the rounds stops (10^(R-1) x eps)
        for (int r = 0; r < q.warm_decades; ++r) { P1.eps_abs *= 10.0; P1.eps_rel *= 10.0; }
        D.nw_follows = 1;  // (newton_kernel writes the outputs of the paths this launch reports SOLVED)
        HIP_TRY(po_launch_solve(form, &s, &D, &P1, h->stream));
        D.nw_follows = 0;
        HIP_TRY(hipEventRecord(h->evp[0], h->stream));
        D.fb_list = static_cast<int *>(h->fb_buf.p);  // (its count: zeroed by scale_kernel)
        // every Newton launch below is ONE launch, or — the constant-class kernels — a pair: that kernel over the paths with the standard row classes, then the kernel
        // without the constants over the others (po_launch_newton_std; the lists live behind nw_keys)
        const auto launch_newton = q.std_classes ? &po_launch_newton_std : &po_launch_newton;
        if (q.std_classes) D.nw_keys = nw_block;
        if (q.sliced) {
            D.nw_state = static_cast<double *>(h->nw_state_buf.p); D.nw_stride = s.park_doubles;
            D.nw_keys = nw_block; D.nw_list = D.nw_keys + B;
            P.ref_nw_slice = h->nw_slice;
            D.nw_phase = 1;
            HIP_TRY(launch_newton(form, &s, &D, &P, h->stream));
            if (q.std_classes) {  // the parked paths in two lists: the standard ones for the constant-class kernel, the others for the kernel without the constants
                const po::StdLists sl = po::std_lists(D.nw_keys, B);
                HIP_TRY(po_launch_nw_sort(D.nw_keys, B, D.nw_list, sl.flag, sl.left2, h->stream));
            } else HIP_TRY(po_launch_nw_sort(D.nw_keys, B, D.nw_list, nullptr, nullptr, h->stream));
            D.nw_phase = 2;
            HIP_TRY(launch_newton(form, &s, &D, &P, h->stream));
            D.nw_phase = 0;
        } else {
            HIP_TRY(launch_newton(form, &s, &D, &P, h->stream));
        }
        HIP_TRY(hipEventRecord(h->evp[1], h->stream));
        h->timed_phases = true;
        // The paths newton_kernel did not certify (rare) are on a device-side work list; newton_fallback_kernel takes them through the later rounds.  Its launch alone
        // costs 0.5 ms whatever its grid (1.2 KB of private segment per lane: the runtime re-provisions scratch for it; 7 % of a BASELINE config-3 solve), so
        // refine_chain = 2 reads the 4-byte count back and launches it only when there is something on the list — the call then returns when the Newton launch has
        // finished (it blocks).  refine_chain = 3: always launched, the call stays asynchronous.
        bool need_fb = true;
        // a stream that is being captured cannot be waited on (the copy below would never run and a synchronise invalidates the capture): always issue the launch then
        hipStreamCaptureStatus cap_st = hipStreamCaptureStatusNone;
        const bool capturing = hipStreamIsCapturing(h->stream, &cap_st) == hipSuccess && cap_st != hipStreamCaptureStatusNone;
        if (q.read_back && !capturing) {
            // the count lands in a pinned word the host SPINS on: a blocking hipStreamSynchronize wakes up through an interrupt — measured 0.5 ms, what the launch it
            // is meant to save costs; falls back to the blocking wait after 20 ms of spinning (a long solve: the wake-up latency no longer matters)
            volatile int *cnt = static_cast<volatile int *>(h->fb_host.p);
            *cnt = -1;
            HIP_TRY(hipMemcpyAsync(const_cast<int *>(cnt), D.fb_list, sizeof(int), hipMemcpyDeviceToHost, h->stream));
            const auto ts0 = std::chrono::steady_clock::now();
            unsigned spins = 0;
            while (*cnt == -1) {
                if ((++spins & 1023u) == 0 && std::chrono::steady_clock::now() - ts0 > std::chrono::milliseconds(20)) { HIP_TRY(hipStreamSynchronize(h->stream)); break; }
#if defined(__x86_64__) || defined(__i386__)
                __builtin_ia32_pause();
#else
                std::this_thread::yield();
#endif
            }
            need_fb = *cnt != 0;
        }
        if (need_fb) HIP_TRY(po_launch_newton_fallback(form, &s, &D, &P, h->stream));
        HIP_TRY(po_launch_finalize_status(D.out_info, B, h->stream));
    } else {
        HIP_TRY(po_launch_solve(form, &s, &D, &P, h->stream));
    }
    if (q.polish) HIP_TRY(po_launch_polish(form, &s, &D, &P, h->stream));
    if (q.no_refine || q.no_polish) HIP_TRY(po_launch_mark_unavailable(D.out_info, B, q.no_refine, q.no_polish, h->stream));
    HIP_TRY(hipEventRecord(h->ev1, h->stream));
    h->timed = true;
    return PO_OK;
}

// ---- step 4 (po_debug_set "debug_cycles"; synchronises): the shader clocks of path 0 and the batch totals of the factorisation counters, on stderr
int dump_cycles(po_handle h, const po::DevBatch &D, int form) PO_REQUIRES(h->mu) {
    long long c4[16];
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(c4, D.dbg_cycles, sizeof(c4), hipMemcpyDeviceToHost));
    std::vector<long long> all(16 * (size_t)D.B);
    HIP_TRY(hipMemcpy(all.data(), D.dbg_cycles, sizeof(long long) * all.size(), hipMemcpyDeviceToHost));
    long long nf = 0, nb = 0;
    double worst = 0;
    for (int b = 0; b < D.B; ++b) {
        nf += all[16 * (size_t)b + 13]; nb += all[16 * (size_t)b + 14];
        double w; std::memcpy(&w, &all[16 * (size_t)b + 15], sizeof(w)); worst = std::fmax(worst, w);
    }
    std::fprintf(stderr, "[po] batch of %d (form %d, N %d, keep %d): %lld scan factorisations, %lld fell back to the sequential chain; worst relative disagreement scan vs recursion %.3e\n", D.B, form, D.N, D.keep, nf, nb, worst);
    std::fprintf(stderr, "[po] path0 cycles: rhs %lld solve %lld update %lld over %lld iterations | solve phases F1 %lld F2 %lld F3B1 %lld B2 %lld B3 %lld | first factorisation: blocks %lld chain %lld | uniform row classes %lld | scan factorisations %lld, fell back to the sequential chain %lld\n",
                 c4[0], c4[1], c4[2], c4[3], c4[4], c4[5], c4[6], c4[7], c4[8], c4[10], c4[11], c4[12], c4[13], c4[14]);
    return PO_OK;
}
}  // namespace

extern "C" {

int po_plan_solve(int form, int N, int keep, int B, int ragged, int refine, int refine_rounds, int refine_extra_rounds, int refine_chain, int polish, int nw_slice,
                  int slice_forced, int fixed_on, int wave_slots, int *out) {
    if (!out) return PO_ERR_INVALID;
    int C;
    PO_TRY(po_problem_dims(form, N, keep, nullptr, nullptr, &C));
    po::SolveShape s;
    po_resolve_solve(form, N, C, keep, &s);
    if (s.lds > po::kLdsLimit) return PO_ERR_UNSUPPORTED;
    po_params p{};
    p.refine = refine; p.refine_rounds = refine_rounds; p.refine_extra_rounds = refine_extra_rounds; p.refine_chain = refine_chain; p.polish = polish;
    const SolveSchedule q = plan_solve(p, s, B, ragged != 0, nw_slice, slice_forced != 0, fixed_on != 0, wave_slots, /* classes_on: the handle's default */ true);
    for (int v : {(int)q.split, (int)q.state, (int)q.polish, (int)q.sliced, (int)q.fixed, (int)q.no_refine, (int)q.no_polish, (int)q.read_back, q.warm_decades}) *out++ = v;
    return PO_OK;
}

int po_solve_batch_device(po_handle h, const po_batch_in *in, const po_batch_out *out) {
    if (!h || !out || !out->states || !out->info) return PO_ERR_INVALID;
    Dims d;
    PO_TRY(validate(in, &d));
    if (in->B == 0) return PO_OK;
    Lock g(h->mu);
    HIP_TRY(hipSetDevice(h->device));
    h->timed_host = false;  // (set again by po_solve_batch when this call is its inner solve: po_last_phase_ms never mixes this solve's events with an older call's)
    po::DevParams P = make_dev_params(h->params, in->formulation, in->keep);
    po::DevBatch D = fill_dev_batch(h, in, out, d);
    const po::SolveShape &s = d.shape;
    SolveSchedule q = plan_solve(h->params, s, in->B, in->n_points != nullptr, h->nw_slice, h->nw_slice_forced, h->fixed_length, h->wave_slots, h->fixed_classes);
    h->fixed_used = D.fixed_len = q.fixed;  // (the one place "fixed" is decided: the launchers read it from D, po_debug_get "fixed_length_used" from the handle)
    PO_TRY(provision(h, s, (size_t)in->B, &q));
    PO_TRY(enqueue(h, in->formulation, s, q, D, P));
    return h->env_cycles ? dump_cycles(h, D, in->formulation) : PO_OK;
}

int po_solve_batch(po_handle h, const po_batch_in *in, const po_batch_out *out) {
    if (!h || !out || !out->states || !out->info) return PO_ERR_INVALID;
    Dims d;
    PO_TRY(validate(in, &d));
    if (in->B == 0) return PO_OK;
    HIP_TRY(hipSetDevice(h->device));
    const size_t B = in->B, N = in->N;
    const bool kpc = in->formulation == PO_KPC;
    if (in->n_points)
        for (size_t b = 0; b < B; ++b)
            if (in->n_points[b] < 2 || in->n_points[b] > in->N) return PO_ERR_INVALID;
    if (in->order) {  // scheduling hint: must be a permutation (checked here; the device-pointer entry trusts its caller)
        std::vector<char> seen(B, 0);
        for (size_t b = 0; b < B; ++b) {
            const int v = in->order[b];
            if (v < 0 || (size_t)v >= B || seen[(size_t)v]) return PO_ERR_INVALID;
            seen[(size_t)v] = 1;
        }
    }
    // the two staging blocks, each a device block and a pinned mirror at the same offsets.  This entry moves them itself (the pack runs under the H2D copies, one D2H)
    Stage I, O;
    const Slot<double> rx = I.in(in->ref_x, B * N), ry = I.in(in->ref_y, B * N), rz = I.in(in->ref_z, B * N), rk = I.in(in->ref_k, B * N), rs = I.in(in->ref_s, B * N);
    const Slot<double> bd = I.in(in->bounds, B * N * 8), x0 = I.in(in->x0, B * 3), gz = I.in(in->goal_z, B);
    const Slot<double> mk = I.in(kpc ? in->max_k : nullptr, B * N), mkp = I.in(kpc ? in->max_kp : nullptr, B * N);
    const Slot<int> np = I.in(in->n_points, B), ord = I.in(in->order, B);
    const Slot<double> os = O.out(out->states, B * N * 5), ox = O.out_opt(out->x, B * (size_t)d.n);
    const Slot<po_info> oi = O.out(out->info, B);
    Lock call(h->call_mu);  // the call lock, as in staged_call (po_handle.hpp); mu is NOT held while the host threads pack and unpack
    hipStream_t st;
    int nthr;
    {
        Lock g(h->mu);
        int rc;
        if ((rc = I.reserve(h, h->in_buf)) || (rc = O.reserve(h, h->out_buf)) || (rc = h->pin_in.ensure(I.bytes())) || (rc = h->pin_out.ensure(O.bytes()))) return rc;
        st = h->stream;
        nthr = h->host_threads > 0 ? h->host_threads : (int)std::min(8u, std::max(1u, std::thread::hardware_concurrency()));
    }
    // ---- pack: caller's (pageable) arrays -> the pinned block, on several host threads; the block goes to the device in slices as they fill ----
    char *dev = static_cast<char *>(h->in_buf.p), *pin = static_cast<char *>(h->pin_in.p);
    std::vector<CopySeg> segs;
    I.each([&](size_t off, size_t bytes, const void *src, void *) { segs.push_back({pin + off, static_cast<const char *>(src), bytes}); });
    double pack_ms, unpack_ms;
    HIP_TRY(hipEventRecord(h->evh[0], st));
    {
        const auto t0 = std::chrono::steady_clock::now();
        // the block in slices of 32 MB: slice k is on its way over PCIe while slice k + 1 is being packed (the alignment gaps between the arrays travel as they are)
        const size_t kSlice = (size_t)32 << 20;
        for (size_t lo = 0; lo < I.bytes(); lo += kSlice) {
            const size_t hi = std::min(I.bytes(), lo + kSlice);
            std::vector<CopySeg> cur;
            for (const CopySeg &sg : segs) {
                const size_t s0 = (size_t)(sg.dst - pin), s1 = s0 + sg.bytes;
                const size_t a0 = std::max(s0, lo), a1 = std::min(s1, hi);
                if (a0 < a1) cur.push_back({pin + a0, sg.src + (a0 - s0), a1 - a0});
            }
            parallel_copy(cur, nthr);
            HIP_TRY(hipMemcpyAsync(dev + lo, pin + lo, hi - lo, hipMemcpyHostToDevice, st));
        }
        pack_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    HIP_TRY(hipEventRecord(h->evh[1], st));
    po_batch_in din = *in;
    din.ref_x = rx; din.ref_y = ry; din.ref_z = rz; din.ref_k = rk; din.ref_s = rs; din.bounds = bd; din.x0 = x0; din.goal_z = gz; din.n_points = np; din.order = ord;
    if (kpc) { din.max_k = mk; din.max_kp = mkp; }
    const po_batch_out dout{os, oi, ox};
    PO_TRY(po_solve_batch_device(h, &din, &dout));
    // ---- D2H into the pinned block (one copy), then unpack on the host threads ----
    char *pout = static_cast<char *>(h->pin_out.p);
    HIP_TRY(hipMemcpyAsync(pout, h->out_buf.p, O.bytes(), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(h->evh[2], st));
    HIP_TRY(hipStreamSynchronize(st));
    {
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<CopySeg> us;
        O.each([&](size_t off, size_t bytes, const void *, void *dst) { us.push_back({static_cast<char *>(dst), pout + off, bytes}); });
        parallel_copy(us, nthr);
        unpack_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    Lock g(h->mu);
    h->host_pack_ms = pack_ms; h->host_unpack_ms = unpack_ms;
    h->timed_host = true;
    return PO_OK;
}

// What the last po_solve_batch (host pointers) spent where, ms: [0] pack + H2D (stream time from the start of the call to the last H2D slice: the pack runs
// under the copies), [1] the solve (= po_last_kernel_ms), [2] D2H, [3] host pack alone (wall), [4] host unpack (wall).  And, for the split scheduling of
// refine = 2, the solve's own phases: [5] equilibration + warm-start launches, [6] the Newton launch, [7] the per-round fallback launches + status sweep (0 otherwise).
int po_last_phase_ms(po_handle h, float *ms8) {
    if (!h || !ms8) return PO_ERR_INVALID;
    Lock g(h->mu);
    if (!h->timed) return PO_ERR_INVALID;
    for (int i = 0; i < 8; ++i) ms8[i] = 0.0f;
    HIP_TRY(hipEventSynchronize(h->ev1));
    HIP_TRY(hipEventElapsedTime(&ms8[1], h->ev0, h->ev1));
    if (h->timed_host) {
        HIP_TRY(hipEventSynchronize(h->evh[2]));
        HIP_TRY(hipEventElapsedTime(&ms8[0], h->evh[0], h->evh[1]));
        HIP_TRY(hipEventElapsedTime(&ms8[2], h->ev1, h->evh[2]));
        ms8[3] = (float)h->host_pack_ms; ms8[4] = (float)h->host_unpack_ms;
    }
    if (h->timed_phases) {
        HIP_TRY(hipEventElapsedTime(&ms8[5], h->ev0, h->evp[0]));
        HIP_TRY(hipEventElapsedTime(&ms8[6], h->evp[0], h->evp[1]));
        HIP_TRY(hipEventElapsedTime(&ms8[7], h->evp[1], h->ev1));
    }
    return PO_OK;
}

int po_last_kernel_ms(po_handle h, float *ms) {
    if (!h || !ms) return PO_ERR_INVALID;
    Lock g(h->mu);
    if (!h->timed) return PO_ERR_INVALID;
    HIP_TRY(hipEventSynchronize(h->ev1));
    HIP_TRY(hipEventElapsedTime(ms, h->ev0, h->ev1));
    return PO_OK;
}

int po_assemble_batch(po_handle h, const po_batch_in *in, double *l, double *u, double *dyn) {
    if (!h || !l || !u || !dyn) return PO_ERR_INVALID;
    if (in && in->n_points) return PO_ERR_INVALID;  // diagnostics work on uniform batches only
    Dims d;
    PO_TRY(validate(in, &d));
    if (in->B == 0) return PO_OK;
    const size_t B = in->B, N = in->N;
    const bool kpc = in->formulation == PO_KPC;
    Stage S;  // the inputs, then the three outputs side by side
    const Slot<double> rx = S.in(in->ref_x, B * N), ry = S.in(in->ref_y, B * N), rz = S.in(in->ref_z, B * N), rk = S.in(in->ref_k, B * N), rs = S.in(in->ref_s, B * N);
    const Slot<double> bd = S.in(in->bounds, B * N * 8), x0 = S.in(in->x0, B * 3), gz = S.in(in->goal_z, B);
    const Slot<double> mk = S.in(kpc ? in->max_k : nullptr, B * N), mkp = S.in(kpc ? in->max_kp : nullptr, B * N);
    const size_t out_from = (S.bytes() + 15) & ~(size_t)15;  // where dl will start
    const Slot<double> dl = S.out(l, B * (size_t)d.m), du = S.out(u, B * (size_t)d.m), dd = S.out(dyn, B * (N - 1) * 3);
    return staged_call(h, S, &po_handle_s::asm_buf, false, [&]() -> int {  // (no device twin: the launch itself, under mu like one)
        Lock g(h->mu);
        po_batch_in din = *in;
        din.ref_x = rx; din.ref_y = ry; din.ref_z = rz; din.ref_k = rk; din.ref_s = rs; din.bounds = bd; din.x0 = x0; din.goal_z = gz;
        if (kpc) { din.max_k = mk; din.max_kp = mkp; }
        HIP_TRY(hipMemsetAsync(dl, 0, S.bytes() - out_from, h->stream));
        const po::DevParams P = make_dev_params(h->params, in->formulation, in->keep);
        const po::DevBatch D = fill_dev_batch(h, &din, nullptr, d);
        HIP_TRY(po_launch_assemble(in->formulation, &D, &P, dl, du, dd, h->stream));
        return PO_OK;
    });
}

int po_scaling_batch(po_handle h, const po_batch_in *in, double *out) {
    if (!h || !out) return PO_ERR_INVALID;
    if (in && in->n_points) return PO_ERR_INVALID;  // diagnostics work on uniform batches only
    Dims d;
    PO_TRY(validate(in, &d));
    if (in->B == 0) return PO_OK;
    const size_t B = in->B, N = in->N;
    Stage S;
    const Slot<double> rs = S.in(in->ref_s, B * N), sc = S.out(out, 64 * B);
    return staged_call(h, S, &po_handle_s::asm_buf, false, [&]() -> int {  // (no device twin: the launch itself, under mu like one)
        Lock g(h->mu);
        po_batch_in din = *in;
        din.ref_s = rs;
        const po::DevParams P = make_dev_params(h->params, in->formulation, in->keep);
        const po::DevBatch D = fill_dev_batch(h, &din, nullptr, d);
        HIP_TRY(po_launch_scale(in->formulation, &D, &P, h->params.scaling, sc, nullptr, nullptr, nullptr, h->stream));  // (diagnostic: no solve follows, nothing to reset)
        return PO_OK;
    });
}

}  // extern "C"
