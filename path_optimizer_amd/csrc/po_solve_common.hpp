// po_solve_common.hpp — what every translation unit that sees the solve kernels shares: the per-path context, the fused solve kernel
// (po_fast.inc), the selection of its shape and THE TABLE of the shapes that are instantiated.  The instantiations themselves are compiled in nineteen objects
// (po_solve_form.hip; po_launch.hpp lists them) that build in parallel; po_kernels.hip holds the dispatcher.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/po_hip.h"
#include "po_device.hpp"
#include "po_launch.hpp"
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

// ---- launch wrappers and the choice of a shape ----
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
// ---- THE TABLE of the shapes that are instantiated: X(formulation, two-level, SPL, NT, NWX, group), one row per shape, matched by EQUALITY on (two, spl, nt, nwx): no
// order, no default.  The group says which objects hold the row (po_launch.hpp: PO_SOLVE_OBJECTS lists the groups of every object; KPC and K: one object of each kind).
// KP: keep 3 / 4 / 5 one lane per chunk, keep 1 / 2 multi-group (4, ., 4 / 5), keep 6 / 7 / 8 role-split, keep 9 .. 16 the WIDE role-split shapes (5 .. 8 stages per lane, one
// wave; as ONE Newton object KP's shapes were the 5-minute pole of the build); KPC: keep 4; K: 2 (N <= 128: one wave) or 4 stages per lane; then the single-level mapping.
// tests/test_shape_table.py reads the rows and compares them with the shapes pick_shape can return.
#define PO_SHAPE_ROWS(X)                                                                                                            \
    X(F_KP, true, 5, 64, 1, kGrpLane) X(F_KP, true, 3, 64, 1, kGrpLane) X(F_KP, true, 3, 128, 1, kGrpLane)                          \
    X(F_KP, true, 4, 64, 1, kGrpLane) X(F_KP, true, 4, 128, 1, kGrpLane)                                                            \
    X(F_KP, true, 4, 64, 4, kGrpMulti) X(F_KP, true, 4, 128, 4, kGrpMulti) X(F_KP, true, 4, 64, 5, kGrpMulti) X(F_KP, true, 4, 128, 5, kGrpMulti) \
    X(F_KP, true, 3, 64, 2, kGrpSplit) X(F_KP, true, 3, 128, 2, kGrpSplit) X(F_KP, true, 4, 64, 2, kGrpSplit) X(F_KP, true, 4, 128, 2, kGrpSplit) \
    X(F_KP, true, 4, 64, 3, kGrpSplit) X(F_KP, true, 4, 128, 3, kGrpSplit)                                                          \
    X(F_KP, true, 5, 64, 2, kGrpW56) X(F_KP, true, 5, 64, 3, kGrpW56) X(F_KP, true, 6, 64, 2, kGrpW56) X(F_KP, true, 6, 64, 3, kGrpW56) \
    X(F_KP, true, 7, 64, 2, kGrpW7) X(F_KP, true, 7, 64, 3, kGrpW7) X(F_KP, true, 8, 64, 2, kGrpW8) X(F_KP, true, 8, 64, 3, kGrpW8)  \
    X(F_K, true, 2, 64, 1, kGrpLane) X(F_K, true, 4, 64, 1, kGrpLane) X(F_K, true, 4, 128, 1, kGrpLane)                             \
    X(F_KPC, true, 4, 64, 1, kGrpLane) X(F_KPC, true, 4, 128, 1, kGrpLane)                                                          \
    X(F_KP, false, 2, 64, 1, kGrpOne) X(F_KP, false, 4, 64, 1, kGrpOne) X(F_KP, false, 4, 128, 1, kGrpOne) X(F_KP, false, 2, 256, 1, kGrpOne) X(F_KP, false, 4, 256, 1, kGrpOne) \
    X(F_KPC, false, 2, 64, 1, kGrpOne) X(F_KPC, false, 4, 64, 1, kGrpOne) X(F_KPC, false, 4, 128, 1, kGrpOne) X(F_KPC, false, 2, 256, 1, kGrpOne) X(F_KPC, false, 4, 256, 1, kGrpOne) \
    X(F_K, false, 2, 64, 1, kGrpOne) X(F_K, false, 4, 64, 1, kGrpOne) X(F_K, false, 4, 128, 1, kGrpOne) X(F_K, false, 2, 256, 1, kGrpOne) X(F_K, false, 4, 256, 1, kGrpOne)
constexpr bool is_shape(const Shape &s, bool two, int spl, int nt, int nwx) { return s.two == two && s.spl == spl && s.nt == nt && s.nwx == nwx; }
// the group of the row that equals (form, s); 0: no row (nothing is instantiated for s)
inline int group_of(int form, const Shape &s) {
#define PO_X(F_, TWO_, SPL_, NT_, NWX_, G_) if (form == F_ && is_shape(s, TWO_, SPL_, NT_, NWX_)) return G_;
    PO_SHAPE_ROWS(PO_X)
#undef PO_X
    return 0;
}
// OSQP's polish: one-lane-per-chunk and multi-group shapes (the role-split shapes of keep 6 .. 16 have no polish kernel: status_polish stays 0 = not attempted, like the single-level mapping)
constexpr bool has_polish_kernel(const Shape &s) { return s.two && s.nwx != 2 && s.nwx != 3; }
// the length-specialised kernels (Fast's NFIX): KP, the shape (SPL 4, NT 64, one lane per chunk), the lengths of the Makefile's PO_FIXED_N (objects of their own, and
// po_kernels.o, get the list as -D'PO_FIXED_LIST(X)=X(200) ...').  Everything else — the general warm-start variant, newton_fallback_kernel, the polish, every other
// shape, ragged batches, unlisted lengths — runs the generic kernels; the layouts are the same.
#ifndef PO_FIXED_LIST
#define PO_FIXED_LIST(X)
#endif
constexpr int kFixSpl = 4, kFixNt = 64;
// the batch is one the fixed instantiations are built for: KP's keep 4 on one lane per chunk, C what path_c() gives a path of N points
inline bool is_fixed_shape(int form, int N, int C, int keep, const Shape &s) { return form == F_KP && keep == kFixSpl && C == (N + keep - 2) / keep && is_shape(s, true, kFixSpl, kFixNt, 1); }
}  // namespace po
