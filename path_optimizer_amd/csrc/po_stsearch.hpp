// po_stsearch.hpp — the station-time search (DESIGN.md sections 29 and 39) as the phases of one workgroup: validation, stations, blocked cells, the layered search
// and the back-trace.  Two kernels are made of them: stplan_kernel (po_stplan.hip; a vehicle that has stopped stays stopped, the plan leaves as v_limit rows) and
// stgo_kernel (po_stgo.hip; a stopped vehicle may pull away again, the plan leaves sampled in time).  They differ in ONE place of the search, the first predecessor
// a moving state looks at (template <bool kResume>), and in one validation rule (kMonotone: stgo looks states up by s).  The definitions are the comments at
// po_stplan_batch and po_stgo_batch in include/po_hip.h; both files match them bit for bit, so both are compiled with -ffp-contract=off (see Makefile) and every
// expression below keeps the order the definitions write.  What is shared with the other readers of agents is po_agents.hpp's.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "../../include/po_hip.h"
#include "../../include/po_pmath.h"
#include "po_agents.hpp"
#include "po_launch.hpp"  // kLdsLimit
#include "po_map.hpp"

namespace po {

constexpr int kStThreads = 512;  // one workgroup per path
static_assert(PO_ST_MAX_STEP + 1 <= 256 && PO_ST_MAX_STATIONS == 128, "back pointers are bytes; a cells row is indexed with >> 7");

// The dynamic LDS of one workgroup, in doubles then ints then bytes; Mb bounds the stations of every path of the call (the launcher computes it from N and stride).
//   A      max(2 * Mb * (U + 1), 12 * Mb) doubles: the circle centres of the stations in phase 1, the two cost layers in phase 2
//   S, Vc  Mb doubles each
//   cell   K * Mb ints, pre K * (Mb + 1) ints (blocked cells in front of station m, per window)
//   bp     K * Mb * (U + 1) bytes
__host__ __device__ constexpr size_t stp_a_doubles(int Mb, int U) { return (size_t)Mb * (2 * (U + 1) > 12 ? 2 * (U + 1) : 12); }
__host__ __device__ constexpr size_t stp_lds_bytes(int K, int Mb, int U) {
    return 8 * (stp_a_doubles(Mb, U) + 2 * (size_t)Mb) + 4 * ((size_t)K * Mb + (size_t)K * (Mb + 1)) + (size_t)K * Mb * (U + 1);
}

// The static LDS the phases share: the agent chunk, the flag of the validation sweep and the chosen plan (nl layers, stations st[0 .. nl], steps u[1 .. nl], cost)
struct StShared {
    double ag[kAgentChunk * kAgentWords];
    int np[kAgentChunk];  // points of the agent; 0: it covers nothing
    int bad, nl, st[PO_ST_MAX_LAYERS + 1], u[PO_ST_MAX_LAYERS + 1];
    double cost;
};
static_assert(stp_lds_bytes(PO_ST_MAX_LAYERS, PO_ST_MAX_STATIONS, PO_ST_MAX_STEP) + sizeof(StShared) <= kLdsLimit, "stplan_kernel's LDS at the limits");

// One path as its workgroup sees it (every field is workgroup-uniform): the rows, the outputs' rows, and the dynamic LDS cut up
struct StPath {
    int b, n, M;
    const double *st;
    double v0;
    int *srow, *crow;
    double *A, *S, *Vc;
    int *cell, *pre;
    unsigned char *bp;
};

// The path of this workgroup and whether it is planned.  Every barrier is reached by the whole workgroup.  kMonotone: s_{i+1} < s_i for some i < n - 1 is one
// more reason not to plan (po_stgo_batch).
template <bool kMonotone>
__device__ __forceinline__ bool st_begin(const DevStSearch &a, StShared &sh, double *lds, StPath &p) {
    const int b = blockIdx.x, tid = threadIdx.x, N = a.N, K = a.K, Mb = a.Mb;
    p.b = b;
    p.n = ag_clamp(a.n_states ? a.n_states[b] : N, N);
    p.st = a.states + (size_t)b * N * 5;
    p.srow = a.station ? a.station + (size_t)b * (PO_ST_MAX_LAYERS + 1) : nullptr;
    p.crow = a.cells ? a.cells + (size_t)b * K * PO_ST_MAX_STATIONS : nullptr;
    p.v0 = a.v0[b];
    p.A = lds; p.S = p.A + stp_a_doubles(Mb, a.U); p.Vc = p.S + Mb;
    p.cell = reinterpret_cast<int *>(p.Vc + Mb); p.pre = p.cell + K * Mb;
    p.bp = reinterpret_cast<unsigned char *>(p.pre + K * (Mb + 1));
    const int n = p.n;
    int M = (n - 1) / a.stride + 1;
    M = M > PO_ST_MAX_STATIONS ? PO_ST_MAX_STATIONS : M;
    p.M = M;
    const bool good = (a.ok ? a.ok[b] != 0 : true) && n >= 2 && ag_finite(p.v0) && p.v0 >= 0 && M >= 2;  // uniform
    if (tid == 0) sh.bad = 0;
    __syncthreads();
    if (good) {
        bool finite = true;
        for (int i = tid; i < n; i += kStThreads) {
            const double *r = p.st + 5 * (size_t)i;
            finite = finite && ag_finite(r[0]) && ag_finite(r[1]) && ag_finite(r[2]) && ag_finite(r[4]);
            if (kMonotone && i < n - 1) finite = finite && !(r[9] < r[4]);
        }
        if (!finite) sh.bad = 1;
    }
    __syncthreads();
    return good && sh.bad == 0;
}

// The plan outputs of a path that is not planned
__device__ __forceinline__ void st_not_planned(const DevStSearch &a, const StPath &p) {
    const int tid = threadIdx.x;
    if (p.crow)
        for (int i = tid; i < a.K * PO_ST_MAX_STATIONS; i += kStThreads) p.crow[i] = -1;
    if (p.srow && tid <= PO_ST_MAX_LAYERS) p.srow[tid] = -1;
    if (tid == 0) {
        a.status[p.b] = 0;
        if (a.ok_out) a.ok_out[p.b] = 0;
        if (a.n_layers) a.n_layers[p.b] = 0;
        if (a.cost) a.cost[p.b] = DBL_MAX;
    }
}

// Stations: s, the cap and the six circle centres (in A: gx at A, gy at A + 6 * Mb); every cell free
__device__ __forceinline__ void st_stations(const DevCar &c, const DevStSearch &a, const StPath &p) {
    const int tid = threadIdx.x, Mb = a.Mb, M = p.M;
    double *gx_l = p.A, *gy_l = p.A + 6 * Mb;
    for (int m = tid; m < M; m += kStThreads) {
        const size_t i = (size_t)m * a.stride;
        const double *r = p.st + 5 * i;
        p.S[m] = r[4];
        double vc = a.v_max;
        if (a.v_cap) {
            const double e = a.v_cap[(size_t)p.b * a.N + i];
            if (e >= 0) vc = ag_min(vc, e);
        }
        p.Vc[m] = vc;
        const double cz = po_pcos(r[2]), sz = po_psin(r[2]);
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            gx_l[6 * m + q] = (c.cx[q] * cz - c.cy[q] * sz) + r[0];
            gy_l[6 * m + q] = (c.cx[q] * sz + c.cy[q] * cz) + r[1];
        }
    }
    const int nc = a.K * M;  // cell ci = k * M + m lives at cell[k * Mb + m]
    for (int ci = tid; ci < nc; ci += kStThreads) p.cell[(ci / M) * Mb + ci % M] = -1;
}

// Phase 1: blocked cells.  Lanes over the K * M cells; a lane holds the six circle centres of its cell's station in registers (the circle loop is unrolled for
// that) and walks the agents of the path's set, which the workgroup moves through LDS kAgentChunk at a time: every lane reads the same agent word, a broadcast.
// Then the counts of blocked cells in front of every station and the cells row.  Returns the number of blocked cells.  On return A is free for the cost layers.
__device__ __forceinline__ int st_blocked(const DevCar &c, const DevStSearch &a, StShared &sh, const StPath &p) {
    const int tid = threadIdx.x, K = a.K, Mb = a.Mb, M = p.M, nc = K * M;
    const double dt = a.dt;
    const double *gx_l = p.A, *gy_l = p.A + 6 * Mb;
    int *cell_l = p.cell, *pre_l = p.pre;
    int lo, hi;
    agent_set_range(a.first, a.set_of, p.b, a.S, a.n_agents, lo, hi);
    for (int c0 = lo; c0 < hi; c0 += kAgentChunk) {
        const int cnt = (hi - c0) < kAgentChunk ? (hi - c0) : kAgentChunk;
        agent_chunk_load<kStThreads>(a.agents + c0, cnt, sh.ag, sh.np);  // (its first barrier: the stations are written; the previous chunk is read)
        for (int cb = 0; cb < nc; cb += kStThreads) {
            const int ci = cb + tid;
            if (ci >= nc) continue;
            const int k = ci / M, m = ci - k * M;
            if (cell_l[k * Mb + m] >= 0) continue;  // an agent of an earlier chunk blocks it: the smallest index is found
            const double tk = (double)k * dt, tk1 = (double)(k + 1) * dt;
            double gx[6], gy[6];
#pragma unroll
            for (int q = 0; q < 6; ++q) { gx[q] = gx_l[6 * m + q]; gy[q] = gy_l[6 * m + q]; }
            int found = -1;
            for (int j = 0; j < cnt && found < 0; ++j) {
                const int np = sh.np[j];
                if (np == 0) continue;
                const double *G = sh.ag + j * kAgentWords;
                const double R = agent_R(G);
                agent_pieces(G, np, tk, tk1, [&](double, double, double axa, double aya, double axb, double ayb) {
#pragma unroll
                    for (int q = 0; q < 6; ++q) {
                        const double gap = agent_gap(gx[q] - axa, gy[q] - aya, gx[q] - axb, gy[q] - ayb, c.cr[q], R);
                        if (gap < a.margin) found = c0 + j;
                    }
                });
            }
            if (found >= 0) cell_l[k * Mb + m] = found;
        }
    }
    __syncthreads();
    if (tid < K) {  // blocked cells in front of station m, per window
        int cntb = 0;
        int *row = pre_l + tid * (Mb + 1);
        for (int m = 0; m < M; ++m) {
            row[m] = cntb;
            cntb += cell_l[tid * Mb + m] >= 0 ? 1 : 0;
        }
        row[M] = cntb;
    }
    __syncthreads();  // from here on A holds the cost layers
    if (p.crow)
        for (int i = tid; i < K * PO_ST_MAX_STATIONS; i += kStThreads) {
            const int k = i >> 7, m = i & (PO_ST_MAX_STATIONS - 1);
            p.crow[i] = m < M ? cell_l[k * Mb + m] : -1;
        }
    int blocked = 0;
    for (int k = 0; k < K; ++k) blocked += pre_l[k * (Mb + 1) + M];
    return blocked;
}

// Phase 2: the search, the choice and the back-trace into sh (nl = 0: no plan).  Lanes over the M * (U + 1) states of a layer, one barrier a layer; wave 0 picks
// the layer's best candidate.  kResume = false: a stopped predecessor (u' == 0) has u == 0 as its one successor, so a moving state starts at u' = 1;
// kResume = true: it starts at u' = 0 like a standing one, and vp = v(j - u, 0) = 0.  Ends with a barrier: sh is readable by the whole workgroup.
template <bool kResume>
__device__ __forceinline__ int st_search(const DevStSearch &a, StShared &sh, const StPath &p) {
    const int tid = threadIdx.x, K = a.K, U1 = a.U + 1, Mb = a.Mb, M = p.M;
    const double dt = a.dt, v0 = p.v0;
    double *A = p.A;
    const double *S_l = p.S, *Vc_l = p.Vc;
    unsigned char *bp_l = p.bp;
    const int nS = M * U1, layer = Mb * U1;
    double best = DBL_MAX;  // wave 0: the choice so far
    int best_k = 0, best_i = 0;
    for (int k = 1; k <= K; ++k) {
        double *cur = A + (k & 1) * layer;
        const double *prev = A + ((k & 1) ^ 1) * layer;
        const int *pre = p.pre + (k - 1) * (Mb + 1);
        for (int s = tid; s < nS; s += kStThreads) {
            const int j = s / U1, u = s - j * U1, pj = j - u;
            double val = DBL_MAX;
            int bp = 0;
            if (pj >= 0 && pj != M - 1 && (k > 1 || pj == 0) && pre[j + 1] - pre[pj] == 0) {
                const double v = (S_l[j] - S_l[pj]) / dt;
                double cc = Vc_l[pj];
                for (int m = pj + 1; m <= j; ++m) cc = ag_min(cc, Vc_l[m]);
                if (u == 0 || (v > 0 && v <= cc)) {
                    const double dv = cc - v, slow = (a.w_slow * dv) * dv;
                    if (k == 1) {
                        const double acc = (v - v0) / dt;
                        if (acc <= a.a_max && acc >= -a.b_max) {
                            const double cand = 0.0 + ((a.w_acc * acc) * acc + slow);
                            if (cand < val) val = cand;
                        }
                    } else {
                        const int umax = a.U < pj ? a.U : pj;
                        for (int up = (!kResume && u > 0) ? 1 : 0; up <= umax; ++up) {
                            const double cp = prev[pj * U1 + up];
                            if (!(cp < DBL_MAX)) continue;
                            const double vp = (S_l[pj] - S_l[pj - up]) / dt;
                            const double acc = (v - vp) / dt;
                            if (!(acc <= a.a_max && acc >= -a.b_max)) continue;
                            const double cand = cp + ((a.w_acc * acc) * acc + slow);
                            if (cand < val) { val = cand; bp = up; }
                        }
                    }
                }
            }
            cur[s] = val;
            bp_l[(size_t)(k - 1) * layer + s] = (unsigned char)bp;
        }
        __syncthreads();
        if (tid < 64) {  // the candidates of this layer in (j, u) order: the arrived states, and every state of layer K
            const int from = k < K ? (M - 1) * U1 : 0;
            double lc = DBL_MAX;
            int li = INT_MAX;
            for (int i = from + tid; i < nS; i += 64) {
                const double v = cur[i];
                if (v < lc) { lc = v; li = i; }
            }
            for (int h = 32; h > 0; h >>= 1) {  // values are never NaN; among equals the smaller index
                const double oc = __shfl_xor(lc, h);
                const int oi = __shfl_xor(li, h);
                if (oc < lc || (oc == lc && oi < li)) { lc = oc; li = oi; }
            }
            if (lc < best) { best = lc; best_k = k; best_i = li; }
        }
        // one barrier a layer is enough: the next layer writes what was `prev` here, which nobody reads any more, and reads `cur`, which is complete
    }
    if (tid == 0) {
        sh.nl = best_k;
        sh.cost = best;
        int j = best_k ? best_i / U1 : 0, u = best_k ? best_i - j * U1 : 0;
        for (int k = best_k; k >= 1; --k) {
            sh.st[k] = j; sh.u[k] = u;
            const int up = bp_l[(size_t)(k - 1) * layer + j * U1 + u];
            j -= u; u = up;
        }
        sh.st[0] = j;
    }
    __syncthreads();
    return sh.nl;
}

// The plan outputs of a path that went through the search: the station row, status, ok_out, n_layers, cost
__device__ __forceinline__ void st_plan_out(const DevStSearch &a, const StShared &sh, const StPath &p, int nl, int blocked) {
    const int tid = threadIdx.x;
    if (p.srow && tid <= PO_ST_MAX_LAYERS) p.srow[tid] = (nl > 0 && tid <= nl) ? sh.st[tid] : -1;
    if (tid == 0) {
        a.status[p.b] = nl == 0 ? 3 : (blocked == 0 ? 1 : 2);
        if (a.ok_out) a.ok_out[p.b] = nl > 0 ? 1 : 0;
        if (a.n_layers) a.n_layers[p.b] = nl;
        if (a.cost) a.cost[p.b] = nl > 0 ? sh.cost : DBL_MAX;
    }
}

}  // namespace po
