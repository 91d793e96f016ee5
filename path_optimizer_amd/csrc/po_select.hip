// po_select.hip — score and select: every candidate path -> eight features and a cost, every group of candidates -> its cheapest feasible
// one, the winners gathered.  The definition is the comment at po_select_batch in include/po_hip.h; this file matches it bit for bit, so it is compiled with
// -ffp-contract=off (see Makefile) and every expression below keeps the order the definition writes.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "../../include/po_hip.h"
#include "../../include/po_pmath.h"
#define PO_MAP_DEVICE_CODE
#include "po_launch.hpp"
#include "po_map.hpp"

namespace po {

// (tests/test_select.py places its path lengths and previous-path sizes around these two: SEL_TILE and PREV_CHUNK there repeat them and change with them)
constexpr int kSelTile = 256;  // states per LDS tile (a multiple of 64: state i stays on lane i mod 64 in every tile)
constexpr int kSelPrev = 256;  // segments of the previous path per LDS chunk (kSelPrev + 1 points)

__device__ __forceinline__ double sel_min(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ double sel_max(double a, double b) { return b > a ? b : a; }
__device__ __forceinline__ bool sel_finite(double v) { return fabs(v) <= DBL_MAX; }  // false for NaN and +-inf
__device__ __forceinline__ int sel_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
// the folds of the definition over the 64 lane partials: lane t < h combines (P_t, P_{t+h}) in that order, so lane 0 ends with P_0
__device__ __forceinline__ double fold_add(double v) {
    for (int h = 32; h > 0; h >>= 1) v = v + __shfl_xor(v, h);
    return v;
}
__device__ __forceinline__ double fold_min(double v) {
    for (int h = 32; h > 0; h >>= 1) v = sel_min(v, __shfl_xor(v, h));
    return v;
}
__device__ __forceinline__ double fold_max(double v) {
    for (int h = 32; h > 0; h >>= 1) v = sel_max(v, __shfl_xor(v, h));
    return v;
}

// gs'[0] = clamp(gs[0], 0, B), gs'[g+1] = clamp(max(gs[g+1], gs'[g]), 0, B): clamping commutes with max, so gs'[g] = clamp(max_{j <= g} gs[j]) — a running maximum.
// One wave: lane t owns entries [t * per, (t + 1) * per), takes their maximum, the lanes' maxima are scanned, and every lane walks its entries again.
__global__ __launch_bounds__(64) void select_groups_kernel(int B, int G, const int *gs, int *out) {
    const int lane = threadIdx.x, cnt = G + 1, per = (cnt + 63) / 64;
    const int lo = lane * per < cnt ? lane * per : cnt, hi = lo + per < cnt ? lo + per : cnt;
    int mx = INT_MIN;
    for (int j = lo; j < hi; ++j) mx = gs[j] > mx ? gs[j] : mx;
    int run = mx;  // inclusive scan of the lane maxima
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(run, d);
        if (lane >= d) run = o > run ? o : run;
    }
    int carry = __shfl_up(run, 1);
    if (lane == 0) carry = INT_MIN;
    for (int j = lo; j < hi; ++j) {
        carry = gs[j] > carry ? gs[j] : carry;
        out[j] = sel_clamp(carry, B);
    }
}

// The group of candidate b in the clamped table: the g with gs'[g] <= b < gs'[g+1], -1 when there is none.  b is wave-uniform, so is the search.
__device__ __forceinline__ int group_of(const int *gs, int G, int b) {
    if (b < gs[0] || b >= gs[G]) return -1;
    int lo = 0, hi = G;  // invariant: gs[lo] <= b < gs[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (gs[mid] <= b) lo = mid; else hi = mid;
    }
    return lo;
}

// One wave per candidate.  Per-state quantities p_i, e_i go to LDS, lane-strided, a tile of kSelTile states (+ the first state of the next tile) at a time; the
// interval terms read entries i and i + 1 from there and rows i and i + 1 of the candidate.  Sums, maximum and minimum are lane partials (state / interval i on lane
// i mod 64, ascending) folded by a butterfly at the end: no atomics.
__global__ __launch_bounds__(64) void select_score_kernel(DevMaps ms, DevCar c, DevSelect a) {
    __shared__ double p_l[kSelTile + 1], e_l[kSelTile + 1], u_l[kSelPrev + 1], v_l[kSelPrev + 1];
    const int b = blockIdx.x, lane = threadIdx.x;
    const DevMap m = map_of(ms, b);
    const double *st = a.states + (size_t)b * a.N * 5;
    const int n = sel_clamp(a.n_states ? a.n_states[b] : a.N, a.N);
    // the previous path of this candidate's group (wave-uniform)
    const double *pv = nullptr;
    int np = 0;
    if (a.prev_states && a.Np > 0) {
        const int g = group_of(a.gs, a.G, b);
        if (g >= 0) {
            np = sel_clamp(a.prev_n ? a.prev_n[g] : a.Np, a.Np);
            pv = a.prev_states + (size_t)g * a.Np * 5;
        }
    }
    const bool has_prev = pv && np >= 2;

    double s1 = 0.0, s2 = 0.0, s5 = 0.0, s7 = 0.0, kmax = 0.0, cmin = DBL_MAX;
    bool finite = true;
    for (int t0 = 0; t0 < n; t0 += kSelTile) {
        // states of this tile: LDS entries lo .. hi (entry i - t0); entry 0 of a later tile is entry kSelTile of the tile before
        const int lo = t0 > 0 ? 1 : 0, hi = (n - 1 - t0) < kSelTile ? (n - 1 - t0) : kSelTile;
        if (t0 > 0) {
            __syncthreads();
            const double cp = p_l[kSelTile], ce = e_l[kSelTile];
            __syncthreads();
            if (lane == 0) { p_l[0] = cp; e_l[0] = ce; }
        }
        for (int li = lane; li <= hi; li += 64) {
            if (li < lo) continue;
            const double *r = st + 5 * (size_t)(t0 + li);
            const double x = r[0], y = r[1], z = r[2], k = r[3], s = r[4];
            finite = finite && sel_finite(x) && sel_finite(y) && sel_finite(z) && sel_finite(k) && sel_finite(s);
            const double cz = po_pcos(z), sz = po_psin(z);
            double ci = 0.0;
#pragma unroll 1
            for (int q = 0; q < 6; ++q) {
                const double gx = (c.cx[q] * cz - c.cy[q] * sz) + x;
                const double gy = (c.cx[q] * sz + c.cy[q] * cz) + y;
                const double cq = map_distance(m, gx, gy) - c.cr[q];
                ci = q == 0 ? cq : sel_min(ci, cq);
            }
            double t = a.d_safe - ci;
            t = t > 0 ? t : 0;
            p_l[li] = t * t;
            e_l[li] = 0.0;
            cmin = sel_min(cmin, ci);
            kmax = sel_max(kmax, fabs(k));
        }
        if (has_prev) {
            for (int c0 = 0; c0 < np - 1; c0 += kSelPrev) {  // segments c0 .. c0 + nseg - 1 of the previous path, points c0 .. c0 + nseg
                const int nseg = (np - 1 - c0) < kSelPrev ? (np - 1 - c0) : kSelPrev;
                __syncthreads();
                for (int j = lane; j <= nseg; j += 64) { u_l[j] = pv[5 * (size_t)(c0 + j)]; v_l[j] = pv[5 * (size_t)(c0 + j) + 1]; }
                __syncthreads();
                for (int li = lane; li <= hi; li += 64) {
                    if (li < lo) continue;
                    const double *r = st + 5 * (size_t)(t0 + li);
                    const double x = r[0], y = r[1];
                    double e = e_l[li];
                    for (int j = 0; j < nseg; ++j) {
                        const double uj = u_l[j], vj = v_l[j];
                        const double dx = u_l[j + 1] - uj, dy = v_l[j + 1] - vj, px = x - uj, py = y - vj;
                        const double L2 = dx * dx + dy * dy, dot = px * dx + py * dy;
                        double t = L2 > 0 ? dot / L2 : 0;
                        t = t < 0 ? 0 : t;
                        t = t > 1 ? 1 : t;
                        const double qx = px - t * dx, qy = py - t * dy;
                        const double D = qx * qx + qy * qy;
                        e = (c0 == 0 && j == 0) ? D : sel_min(e, D);
                    }
                    e_l[li] = e;
                }
            }
        }
        __syncthreads();
        // intervals t0 .. t0 + hi - 1
        for (int li = lane; li < hi; li += 64) {
            const double *r = st + 5 * (size_t)(t0 + li);
            const double k0 = r[3], k1 = r[8], ds = r[9] - r[4];
            const double dk = k1 - k0;
            s1 = s1 + (0.5 * (k0 * k0 + k1 * k1)) * ds;
            s2 = s2 + (ds > 0 ? (dk * dk) / ds : 0);
            s5 = s5 + (0.5 * (p_l[li] + p_l[li + 1])) * ds;
            s7 = s7 + (0.5 * (e_l[li] + e_l[li + 1])) * ds;
        }
    }
    double f[PO_N_FEAT];
    f[PO_FEAT_CURV] = fold_add(s1);
    f[PO_FEAT_CURV_RATE] = fold_add(s2);
    f[PO_FEAT_KMAX] = fold_max(kmax);
    f[PO_FEAT_CLR_MIN] = fold_min(cmin);
    f[PO_FEAT_PROX] = fold_add(s5);
    f[PO_FEAT_DEV_PREV] = fold_add(s7);
    const bool all_finite = !__any(!finite);
    if (lane != 0) return;
    f[PO_FEAT_LENGTH] = 0.0;
    f[PO_FEAT_GOAL] = 0.0;
    if (n > 0) {
        const double *r = st + 5 * (size_t)(n - 1);
        f[PO_FEAT_LENGTH] = r[4];
        if (a.goal) {
            const double gx = a.goal[(size_t)b * a.goal_stride], gy = a.goal[(size_t)b * a.goal_stride + 1];
            f[PO_FEAT_GOAL] = sqrt((r[0] - gx) * (r[0] - gx) + (r[1] - gy) * (r[1] - gy));
        }
    }
    bool feas = (a.ok ? a.ok[b] != 0 : true) && n >= 2 && all_finite;
    double cost = a.w[0] * f[0];
#pragma unroll
    for (int j = 0; j < PO_N_FEAT; ++j) {
        feas = feas && sel_finite(f[j]);
        if (j > 0) cost = cost + a.w[j] * f[j];
        if (a.feat) a.feat[(size_t)b * PO_N_FEAT + j] = f[j];
    }
    feas = feas && f[PO_FEAT_CLR_MIN] >= a.min_clearance && f[PO_FEAT_KMAX] <= a.max_kmax && f[PO_FEAT_GOAL] <= a.max_goal_dist && sel_finite(cost);
    a.cost[b] = feas ? cost : __longlong_as_double(0x7ff0000000000000ll);
}

// One wave per group: lexicographic (cost, index) minimum over the group's candidates and the feasible count, lane-strided and folded by a butterfly; then the same
// wave copies the winner's rows and zeroes the rest of sel_states[g].  A cost below +infinity is a feasible candidate (select_score_kernel writes nothing else).
__global__ __launch_bounds__(64) void select_pick_kernel(DevSelect a) {
    const int g = blockIdx.x, lane = threadIdx.x;
    const int b0 = a.gs[g], b1 = a.gs[g + 1];
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    double bc = inf;
    int bi = INT_MAX, cnt = 0;
    for (int b = b0 + lane; b < b1; b += 64) {
        const double cb = a.cost[b];
        if (cb < inf) {
            ++cnt;
            if (cb < bc || bi == INT_MAX) { bc = cb; bi = b; }
        }
    }
    for (int h = 32; h > 0; h >>= 1) {
        const double oc = __shfl_xor(bc, h);
        const int oi = __shfl_xor(bi, h);
        cnt += __shfl_xor(cnt, h);
        if (oi != INT_MAX && (bi == INT_MAX || oc < bc || (oc == bc && oi < bi))) { bc = oc; bi = oi; }
    }
    const bool found = bi != INT_MAX;
    int n = 0;
    if (found) n = sel_clamp(a.n_states ? a.n_states[bi] : a.N, a.N);
    if (lane == 0) {
        a.best[g] = found ? bi : -1;
        if (a.best_cost) a.best_cost[g] = found ? bc : inf;
        if (a.n_feasible) a.n_feasible[g] = cnt;
        if (a.sel_n) a.sel_n[g] = n;
    }
    if (a.sel_states) {
        double *dst = a.sel_states + (size_t)g * a.N * 5;
        const double *src = a.states + (size_t)(found ? bi : 0) * a.N * 5;
        const size_t rows = 5 * (size_t)a.N, kept = 5 * (size_t)n;
        for (size_t t = lane; t < rows; t += 64) dst[t] = t < kept ? src[t] : 0.0;
    }
}

}  // namespace po

extern "C" hipError_t po_launch_select(const po::DevMaps *m, const po::DevCar *c, const po::DevSelect *a, hipStream_t st) {
    hipLaunchKernelGGL(po::select_groups_kernel, dim3(1), dim3(64), 0, st, a->B, a->G, a->group_start, a->gs);
    hipLaunchKernelGGL(po::select_score_kernel, dim3(a->B), dim3(64), 0, st, *m, *c, *a);
    hipLaunchKernelGGL(po::select_pick_kernel, dim3(a->G), dim3(64), 0, st, *a);
    return hipGetLastError();
}
