// po_stplan.hip — station-time speed planning: per path, the (time window, station) cells the agents of its set block, then a layered
// shortest-path search over (station, stations advanced in the last step) that passes ahead of an agent, eases off behind it or stops, and the v_limit rows that
// hand the plan to po_speed_batch*.  The definition is the comment at po_stplan_batch in include/po_hip.h; this file matches it bit for bit, so it is compiled with
// -ffp-contract=off (see Makefile) and every expression below keeps the order the definition writes.  What it shares with the other readers of agents (the chunk
// through LDS, the walk over an agent's pieces, the closest approach) is po_agents.hpp's.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "../../include/po_hip.h"
#include "../../include/po_pmath.h"
#include "po_agents.hpp"
#include "po_launch.hpp"
#include "po_map.hpp"

namespace po {

constexpr int kStThreads = 512;  // one workgroup per path
static_assert(PO_ST_MAX_STEP + 1 <= 256 && PO_ST_MAX_STATIONS == 128, "back pointers are bytes; a cells row is indexed with >> 7");

// The dynamic LDS of one workgroup, in doubles then ints then bytes; Mb bounds the stations of every path of the call (the launcher computes it from N and stride).
//   A      max(2 * Mb * (U + 1), 12 * Mb) doubles: the circle centres of the stations in phase 1, the two cost layers in phase 2
//   S, Vc  Mb doubles each
//   cell   K * Mb ints, pre K * (Mb + 1) ints (blocked cells in front of station m, per window)
//   bp     K * Mb * (U + 1) bytes
__host__ __device__ inline size_t stp_a_doubles(int Mb, int U) { return (size_t)Mb * (2 * (U + 1) > 12 ? 2 * (U + 1) : 12); }
__host__ __device__ inline size_t stp_lds_bytes(int K, int Mb, int U) {
    return 8 * (stp_a_doubles(Mb, U) + 2 * (size_t)Mb) + 4 * ((size_t)K * Mb + (size_t)K * (Mb + 1)) + (size_t)K * Mb * (U + 1);
}

// One workgroup per path.  Phase 1: lanes over the K * M cells; a lane holds the six circle centres of its cell's station in registers (the circle loop is unrolled
// for that) and walks the agents of the path's set, which the workgroup moves through LDS kAgentChunk at a time: every lane reads the same agent word, a broadcast.
// Phase 2: lanes over the M * (U + 1) states of a layer, one barrier a layer; wave 0 picks the layer's best candidate.  Every barrier is reached by the whole
// workgroup: the loops around them have workgroup-uniform bounds, and the early return of a path that is not planned is uniform too.
__global__ __launch_bounds__(kStThreads) void stplan_kernel(DevCar c, DevStplan a) {
    extern __shared__ double stp_lds[];
    __shared__ double ag_l[kAgentChunk * kAgentWords];
    __shared__ int np_l[kAgentChunk];  // points of the agent; 0: it covers nothing
    __shared__ int bad_l, plan_l[2], plan_st[PO_ST_MAX_LAYERS + 1], plan_u[PO_ST_MAX_LAYERS + 1];
    __shared__ double cost_l;
    const int b = blockIdx.x, tid = threadIdx.x, N = a.N, K = a.K, U1 = a.U + 1, Mb = a.Mb, stride = a.stride;
    const int n = ag_clamp(a.n_states ? a.n_states[b] : N, N);
    const double *st = a.states + (size_t)b * N * 5;
    const double *lin = a.v_limit_in ? a.v_limit_in + (size_t)b * N : nullptr;
    double *lrow = a.v_limit ? a.v_limit + (size_t)b * N : nullptr;
    int *srow = a.station ? a.station + (size_t)b * (PO_ST_MAX_LAYERS + 1) : nullptr, *crow = a.cells ? a.cells + (size_t)b * K * PO_ST_MAX_STATIONS : nullptr;
    const double v0 = a.v0[b], dt = a.dt;

    double *A = stp_lds, *S_l = A + stp_a_doubles(Mb, a.U), *Vc_l = S_l + Mb;
    int *cell_l = reinterpret_cast<int *>(Vc_l + Mb), *pre_l = cell_l + K * Mb;
    unsigned char *bp_l = reinterpret_cast<unsigned char *>(pre_l + K * (Mb + 1));

    int M = (n - 1) / stride + 1;
    M = M > PO_ST_MAX_STATIONS ? PO_ST_MAX_STATIONS : M;
    const bool good = (a.ok ? a.ok[b] != 0 : true) && n >= 2 && ag_finite(v0) && v0 >= 0 && M >= 2;  // uniform
    if (tid == 0) bad_l = 0;
    __syncthreads();
    if (good) {
        bool finite = true;
        for (int i = tid; i < n; i += kStThreads) {
            const double *r = st + 5 * (size_t)i;
            finite = finite && ag_finite(r[0]) && ag_finite(r[1]) && ag_finite(r[2]) && ag_finite(r[4]);
        }
        if (!finite) bad_l = 1;
    }
    __syncthreads();
    const bool planned = good && bad_l == 0;

    if (!planned) {  // (uniform)
        if (lrow)
            for (int i = tid; i < N; i += kStThreads) lrow[i] = lin ? lin[i] : -1.0;
        if (crow)
            for (int i = tid; i < K * PO_ST_MAX_STATIONS; i += kStThreads) crow[i] = -1;
        if (srow && tid <= PO_ST_MAX_LAYERS) srow[tid] = -1;
        if (tid == 0) {
            a.status[b] = 0;
            if (a.ok_out) a.ok_out[b] = 0;
            if (a.n_layers) a.n_layers[b] = 0;
            if (a.cost) a.cost[b] = DBL_MAX;
        }
        return;
    }

    // ---- stations: s, the cap and the six circle centres ----
    double *gx_l = A, *gy_l = A + 6 * Mb;
    for (int m = tid; m < M; m += kStThreads) {
        const size_t i = (size_t)m * stride;
        const double *r = st + 5 * i;
        S_l[m] = r[4];
        double vc = a.v_max;
        if (a.v_cap) {
            const double e = a.v_cap[(size_t)b * N + i];
            if (e >= 0) vc = ag_min(vc, e);
        }
        Vc_l[m] = vc;
        const double cz = po_pcos(r[2]), sz = po_psin(r[2]);
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            gx_l[6 * m + q] = (c.cx[q] * cz - c.cy[q] * sz) + r[0];
            gy_l[6 * m + q] = (c.cx[q] * sz + c.cy[q] * cz) + r[1];
        }
    }
    const int nc = K * M;  // cell ci = k * M + m lives at cell_l[k * Mb + m]
    for (int ci = tid; ci < nc; ci += kStThreads) cell_l[(ci / M) * Mb + ci % M] = -1;

    // ---- phase 1: blocked cells ----
    int lo, hi;
    agent_set_range(a.first, a.set_of, b, a.S, a.n_agents, lo, hi);
    for (int c0 = lo; c0 < hi; c0 += kAgentChunk) {
        const int cnt = (hi - c0) < kAgentChunk ? (hi - c0) : kAgentChunk;
        agent_chunk_load<kStThreads>(a.agents + c0, cnt, ag_l, np_l);  // (its first barrier: the stations are written; the previous chunk is read)
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
                const int np = np_l[j];
                if (np == 0) continue;
                const double *G = ag_l + j * kAgentWords;
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
    if (crow)
        for (int i = tid; i < K * PO_ST_MAX_STATIONS; i += kStThreads) {
            const int k = i >> 7, m = i & (PO_ST_MAX_STATIONS - 1);
            crow[i] = m < M ? cell_l[k * Mb + m] : -1;
        }
    int blocked = 0;
    for (int k = 0; k < K; ++k) blocked += pre_l[k * (Mb + 1) + M];

    // ---- phase 2: the search ----
    const int nS = M * U1, layer = Mb * U1;
    double best = DBL_MAX;  // wave 0: the choice so far
    int best_k = 0, best_i = 0;
    for (int k = 1; k <= K; ++k) {
        double *cur = A + (k & 1) * layer;
        const double *prev = A + ((k & 1) ^ 1) * layer;
        const int *pre = pre_l + (k - 1) * (Mb + 1);
        for (int s = tid; s < nS; s += kStThreads) {
            const int j = s / U1, u = s - j * U1, p = j - u;
            double val = DBL_MAX;
            int bp = 0;
            if (p >= 0 && p != M - 1 && (k > 1 || p == 0) && pre[j + 1] - pre[p] == 0) {
                const double v = (S_l[j] - S_l[p]) / dt;
                double cc = Vc_l[p];
                for (int m = p + 1; m <= j; ++m) cc = ag_min(cc, Vc_l[m]);
                if (u == 0 || (v > 0 && v <= cc)) {
                    const double dv = cc - v, slow = (a.w_slow * dv) * dv;
                    if (k == 1) {
                        const double acc = (v - v0) / dt;
                        if (acc <= a.a_max && acc >= -a.b_max) {
                            const double cand = 0.0 + ((a.w_acc * acc) * acc + slow);
                            if (cand < val) val = cand;
                        }
                    } else {
                        const int umax = a.U < p ? a.U : p;
                        for (int up = u > 0 ? 1 : 0; up <= umax; ++up) {  // (a stopped predecessor, up == 0, has u == 0 as its one successor)
                            const double cp = prev[p * U1 + up];
                            if (!(cp < DBL_MAX)) continue;
                            const double vp = (S_l[p] - S_l[p - up]) / dt;
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
        plan_l[0] = best_k;
        cost_l = best;
        int j = best_k ? best_i / U1 : 0, u = best_k ? best_i - j * U1 : 0;
        for (int k = best_k; k >= 1; --k) {
            plan_st[k] = j; plan_u[k] = u;
            const int up = bp_l[(size_t)(k - 1) * layer + j * U1 + u];
            j -= u; u = up;
        }
        plan_st[0] = j;
    }
    __syncthreads();
    const int nl = plan_l[0];
    if (srow && tid <= PO_ST_MAX_LAYERS) srow[tid] = (nl > 0 && tid <= nl) ? plan_st[tid] : -1;
    if (lrow)
        for (int i = tid; i < N; i += kStThreads) {
            const double L = lin ? lin[i] : -1.0;
            double val = L;
            if (nl > 0 && i < n) {
                const int m = i / stride;
                if (m >= plan_st[nl]) {
                    if (plan_u[nl] == 0) val = 0.0;
                } else {
                    int k = 0;
                    while (k < nl - 1 && !(plan_st[k] <= m && m < plan_st[k + 1])) ++k;  // (station[0] = 0 <= m < station[nl], stations do not decrease)
                    const double V = (S_l[plan_st[k + 1]] - S_l[plan_st[k]]) / dt;
                    val = L >= 0 ? ag_min(L, V) : V;
                }
            }
            lrow[i] = val;
        }
    if (tid == 0) {
        const int status = nl == 0 ? 3 : (blocked == 0 ? 1 : 2);
        a.status[b] = status;
        if (a.ok_out) a.ok_out[b] = nl > 0 ? 1 : 0;
        if (a.n_layers) a.n_layers[b] = nl;
        if (a.cost) a.cost[b] = nl > 0 ? cost_l : DBL_MAX;
    }
}

}  // namespace po

extern "C" hipError_t po_launch_stplan(const po::DevCar *c, const po::DevStplan *a, hipStream_t st) {
    const size_t lds = po::stp_lds_bytes(a->K, a->Mb, a->U);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&po::stplan_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(po::stplan_kernel, dim3(a->B), dim3(po::kStThreads), lds, st, *c, *a);
    return hipGetLastError();
}
