// po_kernels.hip — gfx950 (MI355X) kernels of libpo_hip.so.
//
//   scale_kernel    (po_scale.hpp)  per-path class-level Ruiz equilibration (OSQP's default scaling = 10)
//   solve_kernel_fast (po_fast.inc) the fused batched QP solve: assembly + factorisation + ADMM + output map
//                                   in ONE launch, per-path state resident in VGPRs / LDS
//   assemble_kernel                 diagnostic: the assembled bounds / data-dependent A entries in the
//                                   reference row order, for bit-exact comparison with the oracle
// and the DISPATCHER of the solve kernels, which live in objects of their own (po_solve_form.hip): po_resolve_solve resolves the shape of a batch ONCE per call of a solve
// entry (po_solve.cpp) into a SolveShape (po_launch.hpp) — the shape, its LDS bytes, the group of the row of the table of shapes (po_solve_common.hpp) that equals it,
// and every size and capability the host asks about — and the launches take that: the list of objects (po_launch.hpp) names the one object to call.  The exported size
// and capability queries (po_polish_state_doubles, ...) read the same resolution.
//
// Replaces, per path, the work behind /root/reference/src/solver/solver.cpp:46-77 (setHessianMatrix,
// setConstraintMatrix, osqp_setup, osqp_solve, getOptimizedPath).
#include "po_solve_common.hpp"

namespace po {

// diagnostic assembly kernel: l,u in reference row order + data-dependent A entries per transition
template <int F> __global__ __launch_bounds__(64) void assemble_kernel(DevBatch in, DevParams P, double *l, double *u, double *dyn) {
    using T = FormTraits<F>;
    extern __shared__ double smem[];
    const int b = blockIdx.x;
    Ctx<F> cx(P, in, smem, b);
    const int N = cx.N, C = cx.C;
    double *lb = l + (size_t)b * in.m, *ub = u + (size_t)b * in.m;
    for (int j = cx.lane; j < N; j += 64) {
        const StageIn si = cx.stage_in(j);
        AsmFn<F> fn{lb, ub, j, N, C, 0};
        local_rows<F>(si, P, fn);
        if (T::NEND && si.last) { fn.kind = 1; end_rows<F>(si, P, fn); }
        double bin[3];
        if (j == 0) cx.init_bounds(bin);
        else {
            const Dyn<F> d = cx.dyn(j - 1);
#pragma unroll
            for (int r = 0; r < T::NDYN; ++r) bin[r] = d.b[r];
            double *dd = dyn + ((size_t)b * (N - 1) + (j - 1)) * 3;
            if constexpr (F == F_K) { dd[0] = d.f[0][0]; dd[1] = d.f[1][1]; dd[2] = d.f[0][2]; }
            else { dd[0] = d.f[0][1]; dd[1] = d.f[1][0]; dd[2] = d.beta[2]; }
        }
#pragma unroll
        for (int r = 0; r < T::NDYN; ++r) { lb[T::NDYN * j + r] = bin[r]; ub[T::NDYN * j + r] = bin[r]; }
        if constexpr (F == F_K) {
            if (si.last) { /* delta_{N-1} has no box row */ }
        }
    }
    if constexpr (T::HAS_U)
        for (int c = cx.lane; c < C; c += 64) {
            AsmFn<F> fn{lb, ub, c, N, C, 2};
            const double mkp = (F == F_KPC) ? in.max_kp[cx.po + c] : 0.0;
            ctl_rows<F>(mkp, fn);
        }
}

}  // namespace po

namespace po {
// After the launches of a solve that hands paths from launch to launch (the Newton refinement's rounds): no internal "in flight" status may reach the caller
// (a path that a malformed caller-side order skipped): anything at or below kStatusDeferred becomes UNSOLVED.
__global__ void finalize_status_kernel(po_info *info, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B && info[b].status <= kStatusDeferred) { info[b].status = PO_STATUS_UNSOLVED; info[b].status_polish = 0; }
}
// A caller that asked for the Newton refinement (po_params.refine = 2) or the polish on a shape that has no kernel for it (the single-level mapping; polish: also the role-split
// shapes) can SEE that: status_refine / status_polish = -2 (PO_NOT_AVAILABLE) on every path instead of 0, which also means "off" (include/po_hip.h, ABI 6).
__global__ void mark_unavailable_kernel(po_info *info, int B, int refine, int polish) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) {
        if (refine) info[b].status_refine = PO_NOT_AVAILABLE;
        if (polish) info[b].status_polish = PO_NOT_AVAILABLE;
    }
}
}  // namespace po
extern "C" hipError_t po_launch_mark_unavailable(po_info *info, int B, int refine, int polish, hipStream_t st) {
    hipLaunchKernelGGL(po::mark_unavailable_kernel, dim3((B + 255) / 256), dim3(256), 0, st, info, B, refine, polish);
    return hipGetLastError();
}
// ---- the dispatcher of the solve kernels.  The shape of a batch is resolved ONCE per call of a solve entry (po_resolve_solve, below); a launch calls the ONE object that
// holds that formulation, kind and group (po_launch.hpp) with the shape and its LDS bytes; what that entry returns is the result.
namespace po {
namespace {
using Entry = hipError_t(int, const Shape &, size_t, const DevBatch *, const DevParams *, hipStream_t);
struct Object { Entry *entry; int form, kind, groups; };
#define PO_X(name, form, kind, groups) {&name, form, kind, groups},
const Object kObjects[] = {PO_SOLVE_OBJECTS(PO_X)};
#undef PO_X
template <int F, bool TWO, int SPL, int NT, int NWX> struct RowSizes { static constexpr int state = 0, park = 0; };  // the single-level mapping: neither Newton nor polish
template <int F, int SPL, int NT, int NWX> struct RowSizes<F, true, SPL, NT, NWX> {
    static constexpr int state = Fast<F, SPL, NT, true, NWX>::kStateDoubles * NT, park = Fast<F, SPL, NT, true, NWX>::kParkDoubles * NT + kNwParkScalars;
};
hipError_t call(int form, int kind, int launch, const SolveShape &r, const DevBatch *in, const DevParams *P, hipStream_t st) {
    if (!r.nt || r.lds > kLdsLimit) return hipErrorInvalidValue;
    const Shape s{.nt = r.nt, .spl = r.spl, .two = r.two != 0, .nwx = r.nwx};
    for (const Object &o : kObjects)
        if (o.form == form && o.kind == kind && (o.groups & r.group) && o.entry) return o.entry(launch, s, r.lds, in, P, st);
    return hipErrorNotSupported;  // no row equals the shape, or (dev builds) the object is not linked
}
// a listed length (DevBatch::fixed_len, set from the schedule's `fixed`): the kernels compiled for that length
bool fixed(const SolveShape &r, const DevBatch *in) { return r.fixed && in->fixed_len && in->n_points == nullptr; }
}  // namespace
}  // namespace po
// Two launches on the same stream for the two-level mapping: the uniform-row-class variant first (solves what it can, defers the rest; a listed length: the one compiled
// for that length), then the general variant, which solves only what the first deferred (po_fast.inc, solve_kernel_fast).  Shapes without a uniform variant (the
// single-level mapping, K on multi-wave blocks): the general variant alone.
extern "C" hipError_t po_launch_solve(int form, const po::SolveShape *s, const po::DevBatch *in, const po::DevParams *P, hipStream_t st) {
    using namespace po;
    hipError_t e;
    DevBatch copy = *in;
    copy.only_deferred = 0;
    if (s->uni && (e = call(form, fixed(*s, in) ? kObjFixUni : kObjUni, kLaunchSolve, *s, &copy, P, st)) != hipSuccess) return e;
    copy.only_deferred = s->uni ? 1 : 0;
    return call(form, kObjGen, kLaunchSolve, *s, &copy, P, st);
}
// no internal "in flight" status reaches the caller (finalize_status_kernel)
extern "C" hipError_t po_launch_finalize_status(po_info *info, int B, hipStream_t st) {
    hipLaunchKernelGGL(po::finalize_status_kernel, dim3((B + 255) / 256), dim3(256), 0, st, info, B);
    return hipGetLastError();
}

// the launches that pick up the state block of a two-level shape: the Newton refinement of round 0 (po_params.refine = 2; a listed length: the kernel compiled for it), the
// fallback launch for what it hands back, and the polish
static hipError_t launch_two_level(int form, int launch, const po::SolveShape *s, const po::DevBatch *in, const po::DevParams *P, hipStream_t st) {
    using namespace po;
    if (!s->two) return hipErrorInvalidValue;
    if (launch == kLaunchPolish && !s->polish) return hipSuccess;
    const int kind = (launch == kLaunchNewton && fixed(*s, in)) ? (in->nw_phase == 2 ? kObjFixNewton2 : kObjFixNewton1) : (launch == kLaunchPolish ? kObjGen : kObjNewton);
    return call(form, kind, launch, *s, in, P, st);
}
extern "C" hipError_t po_launch_newton(int form, const po::SolveShape *s, const po::DevBatch *in, const po::DevParams *P, hipStream_t st) { return launch_two_level(form, po::kLaunchNewton, s, in, P, st); }
// The Newton launch of a listed length as a pair (phase by DevBatch::nw_phase, like po_launch_newton): the constant-class kernel over the paths
// whose row classes are the standard ones, then the kernel without the constants over the others.  The first (or only) phase is preceded by the launch that decides
// which are which (newton_std_select_kernel) and gives each kernel its paths as its `order` (-1: that workgroup leaves); the second phase takes the two lists the
// caller has sorted the parked paths into (po_launch_nw_sort by StdLists::flag: in->nw_list and StdLists::left2).  The caller has set in->nw_keys to the block that
// holds the lists (std_lists) and scale_kernel has reset them.  Only for a batch po_launch_newton would run fixed.
extern "C" hipError_t po_launch_newton_std(int form, const po::SolveShape *s, const po::DevBatch *in, const po::DevParams *P, hipStream_t st) {
    using namespace po;
    if (!s->two || !fixed(*s, in) || !in->nw_keys) return hipErrorInvalidValue;
    const bool second = in->nw_phase == 2;
    const StdLists sl = std_lists(in->nw_keys, in->B);
    hipError_t e;
    DevBatch std_ = *in, rest = *in;
    if (second) rest.nw_list = sl.left2;
    else {
        if ((e = call(form, kObjFixNewtonStd1, kLaunchStdSelect, *s, in, P, st)) != hipSuccess) return e;
        std_.order = sl.order; rest.order = sl.left1;
    }
    if ((e = call(form, second ? kObjFixNewtonStd2 : kObjFixNewtonStd1, kLaunchNewtonStd, *s, &std_, P, st)) != hipSuccess) return e;
    return call(form, second ? kObjFixNewton2 : kObjFixNewton1, kLaunchNewton, *s, &rest, P, st);
}
extern "C" hipError_t po_launch_newton_fallback(int form, const po::SolveShape *s, const po::DevBatch *in, const po::DevParams *P, hipStream_t st) { return launch_two_level(form, po::kLaunchFallback, s, in, P, st); }
// OSQP's polish (po_params.polish) on the paths the two solve launches reported solved; same stream, after them (a shape without a polish kernel: nothing to do)
extern "C" hipError_t po_launch_polish(int form, const po::SolveShape *s, const po::DevBatch *in, const po::DevParams *P, hipStream_t st) { return launch_two_level(form, po::kLaunchPolish, s, in, P, st); }
namespace po {
// the parked paths (keys[b] >= 0) in descending key order, ties in path order (a stable counting sort: deterministic): list[0] = count, list[1 ..] = path ids.
// One workgroup of kNwSortThreads threads, thread t owns the contiguous range of paths [t * per, (t + 1) * per).
constexpr int kNwSortThreads = 256;  // (kNwKeys = 32 keys x 257 counters = 33 KB of LDS)
// flag != nullptr (the split between the constant-class second launch and the one without the constants, po_launch_newton_std): TWO workgroups, the first lists the
// paths with flag[b] == 1 in list, the second those with flag[b] == 0 in list2 — side by side, in the time of one
__global__ __launch_bounds__(kNwSortThreads) void nw_sort_kernel(const int *keys, int B, int *list, const int *flag, int *list2) {
    const int want = blockIdx.x == 0 ? 1 : 0;
    if (blockIdx.x != 0) list = list2;
    auto key = [&](int b) { return (flag == nullptr || flag[b] == want) ? keys[b] : -1; };
    // (round 6) a thread's counters live in its own COLUMN of the LDS table (no conflicts, one read-modify-write per path instead of a 32-way compare over registers), its
    // first 16 keys are loaded at once and kept for the scatter pass, and the rows are scanned by whole waves: 22 -> ~10 us for 4 096 paths
    __shared__ int cnt[kNwKeys][kNwSortThreads + 1];
    __shared__ int rowbase[kNwKeys];
    const int t = threadIdx.x, per = (B + kNwSortThreads - 1) / kNwSortThreads, lo = t * per, hi = min(B, lo + per);
    constexpr int kCache = 16;
    int kc[kCache];
#pragma unroll
    for (int i = 0; i < kCache; ++i) kc[i] = (lo + i < hi) ? key(lo + i) : -1;
#pragma unroll
    for (int k = 0; k < kNwKeys; ++k) cnt[k][t] = 0;
#pragma unroll
    for (int i = 0; i < kCache; ++i)
        if (kc[i] >= 0) cnt[kc[i] < kNwKeys ? kc[i] : kNwKeys - 1][t] += 1;
    for (int b = lo + kCache; b < hi; ++b) {
        const int k = key(b);
        if (k >= 0) cnt[k < kNwKeys ? k : kNwKeys - 1][t] += 1;
    }
    __syncthreads();
    // exclusive prefix over (key descending, thread ascending): per key a scan of its row of kNwSortThreads counters (lane l takes kNwSortThreads / 64 consecutive counters, a
    // 6-step shuffle scan over the lanes' sums), then the rows are offset by the totals of the higher keys
    {
        constexpr int kPerLane = kNwSortThreads / 64, kWaves = kNwSortThreads / 64;
        const int lane = t & 63, wv = t >> 6;
        for (int k = wv; k < kNwKeys; k += kWaves) {
            int v[kPerLane], sum = 0;
#pragma unroll
            for (int i = 0; i < kPerLane; ++i) { v[i] = cnt[k][lane * kPerLane + i]; sum += v[i]; }
            int incl = sum;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(incl, d, 64); if (lane >= d) incl += o; }
            int run = incl - sum;
#pragma unroll
            for (int i = 0; i < kPerLane; ++i) { cnt[k][lane * kPerLane + i] = run; run += v[i]; }
            if (lane == 63) cnt[k][kNwSortThreads] = incl;
        }
    }
    __syncthreads();
    if (t < kNwKeys) {
        int run = 0;
        for (int j = kNwKeys - 1; j > t; --j) run += cnt[j][kNwSortThreads];
        rowbase[t] = run;
        if (t == 0) list[0] = run + cnt[0][kNwSortThreads];
    }
    __syncthreads();
    auto place = [&](int b, int k) {  // (own column again: the next free position of this thread's paths with this key)
        const int kk = k < kNwKeys ? k : kNwKeys - 1;
        const int pos = rowbase[kk] + cnt[kk][t];
        cnt[kk][t] += 1;
        list[1 + pos] = b;
    };
#pragma unroll
    for (int i = 0; i < kCache; ++i)
        if (kc[i] >= 0) place(lo + i, kc[i]);
    for (int b = lo + kCache; b < hi; ++b) {
        const int k = key(b);
        if (k >= 0) place(b, k);
    }
}

}  // namespace po
// sliced Newton launches: the parked paths ordered by expected remaining work (one small workgroup; ~10 us)
extern "C" hipError_t po_launch_nw_sort(const int *keys, int B, int *list, const int *flag, int *list2, hipStream_t st) {
    hipLaunchKernelGGL(po::nw_sort_kernel, dim3(flag ? 2 : 1), dim3(po::kNwSortThreads), 0, st, keys, B, list, flag, list2);
    return hipGetLastError();
}
// ---- the resolution of a batch's shape, and the queries that read it: functions of the resolved shape and of class constants of its table row; no object is asked
extern "C" int po_resolve_solve(int form, int N, int C, int keep, po::SolveShape *r) {
    using namespace po;
    *r = SolveShape{};
    r->lds = (size_t)1 << 30;
    Shape s;
    // K has no held controls: its shape is that of C = 0, whatever the caller's C (po_problem_dims: N - 1) — normalised here and nowhere else ...
    if (!resolve_shape(form, N, form == F_K ? 0 : C, keep, &s)) return 0;
    r->nt = s.nt; r->spl = s.spl; r->two = s.two; r->nwx = s.nwx;
    // ... but its LDS bytes are those of the caller's C: the single-level layout (LayoutF, !two) keeps room for C controls in every formulation, K's single-level batches
    // (N > 512) have always been launched with, and refused by, that size, and tests/golden/shape_queries.json pins it.  (The two-level layout does not read C.)
    r->lds = lds_of(form, N, C, s);
    r->group = group_of(form, s);
#ifdef PO_DEV_HEADLINE  // (the KP objects of `make dev` hold their one shape whatever its group: the first linked object of the kind is asked)
    if (form == F_KP && r->group) r->group = ~0;
#endif
    r->uni = form == F_K ? has_uni_variant<F_K>(s) : has_uni_variant<F_KP>(s);
    r->polish = has_polish_kernel(s);  // (the role-split shapes of keep 6 .. 16 and the single-level mapping have none)
    bool listed = false;  // a length-specialised instantiation for a (non-ragged) batch of this shape?  (KP only; this object is built with the list, PO_FIXED_LIST)
#define PO_X(N_) listed = listed || N == N_;
    PO_FIXED_LIST(PO_X)
#undef PO_X
    r->fixed = listed && is_fixed_shape(form, N, C, keep, s) && r->lds <= kLdsLimit;
#define PO_X(F_, TWO_, SPL_, NT_, NWX_, G_) if (form == F_ && is_shape(s, TWO_, SPL_, NT_, NWX_)) { r->state_doubles = RowSizes<F_, TWO_, SPL_, NT_, NWX_>::state; r->park_doubles = RowSizes<F_, TWO_, SPL_, NT_, NWX_>::park; }
    PO_SHAPE_ROWS(PO_X)
#undef PO_X
    return 1;
}
static po::SolveShape resolved(int form, int N, int C, int keep) { po::SolveShape r; po_resolve_solve(form, N, C, keep, &r); return r; }
// dynamic LDS bytes of the batch's kernels (1 GB: no shape)
extern "C" size_t po_lds_bytes(int form, int N, int C, int keep) { return resolved(form, N, C, keep).lds; }
// threads per path of the shape this batch runs in (0: unsupported)
extern "C" int po_shape_threads(int form, int N, int C, int keep) { return resolved(form, N, C, keep).nt; }
// doubles per path of the state block the solve kernels leave for the Newton refinement and the polish (0: shape without either: the single-level mapping)
extern "C" int po_polish_state_doubles(int form, int N, int C, int keep) { return resolved(form, N, C, keep).state_doubles; }
// doubles per path of the block a PARKED Newton path lives in between the two sliced launches (Fast::park_io + kNwParkScalars)
extern "C" int po_newton_park_doubles(int form, int N, int C, int keep) { return resolved(form, N, C, keep).park_doubles; }
extern "C" int po_has_polish_kernel(int form, int N, int C, int keep) { return resolved(form, N, C, keep).polish; }
extern "C" int po_has_fixed_length(int form, int N, int C, int keep) { return resolved(form, N, C, keep).fixed; }

// nw_keys ([B]) / fb_count (one int) / std_block (the lists of the constant-class Newton kernels: std_lists, po_device.hpp), when set: reset by the same launch
// (scale_kernel) — the solve needs no fill of its own between its launches
extern "C" hipError_t po_launch_scale(int form, const po::DevBatch *in, const po::DevParams *P, int passes, double *sc, int *nw_keys, int *fb_count, int *std_block,
                                      hipStream_t st) {
    using namespace po;
    const int bs = 64, gs = (in->B + bs - 1) / bs;
    if (form == F_KP) hipLaunchKernelGGL(scale_kernel<F_KP>, dim3(gs), dim3(bs), 0, st, *in, *P, passes, sc, nw_keys, fb_count, std_block);
    else if (form == F_KPC) hipLaunchKernelGGL(scale_kernel<F_KPC>, dim3(gs), dim3(bs), 0, st, *in, *P, passes, sc, nw_keys, fb_count, std_block);
    else hipLaunchKernelGGL(scale_kernel<F_K>, dim3(gs), dim3(bs), 0, st, *in, *P, passes, sc, nw_keys, fb_count, std_block);
    return hipGetLastError();
}

extern "C" hipError_t po_launch_assemble(int form, const po::DevBatch *in, const po::DevParams *P, double *l, double *u, double *dyn, hipStream_t st) {
    using namespace po;
    if (form == F_KP) hipLaunchKernelGGL(assemble_kernel<F_KP>, dim3(in->B), dim3(64), 0, st, *in, *P, l, u, dyn);
    else if (form == F_KPC) hipLaunchKernelGGL(assemble_kernel<F_KPC>, dim3(in->B), dim3(64), 0, st, *in, *P, l, u, dyn);
    else hipLaunchKernelGGL(assemble_kernel<F_K>, dim3(in->B), dim3(64), 0, st, *in, *P, l, u, dyn);
    return hipGetLastError();
}
