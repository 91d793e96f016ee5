// po_agents.hpp — what the kernels that read po_agent records share: po_dynamic.hip, po_stplan.hip and po_nudge.hip move the agents of a
// path's set through LDS a chunk at a time and walk each agent's pieces over a time window; po_trajectory.hip, which writes records, takes the constants.  The
// pieces and windows are defined once, in the comment at po_dynamic_batch in include/po_hip.h, and the kernels are compared with that definition bit for bit: their
// objects are compiled with -ffp-contract=off (see Makefile) and every expression here keeps the order the definition writes.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>

#include "../../include/po_hip.h"

namespace po {

// (tests/test_dynamic.py, test_stplan.py and test_nudge.py place their agent counts around this: their *_CHUNK repeat it and change with it)
constexpr int kAgentChunk = 32;                    // agents per LDS chunk
constexpr int kAgentWords = sizeof(po_agent) / 8;  // an agent as 8-byte words: (n_pts, flags), radius, t[8], x[8], y[8]
static_assert(sizeof(po_agent) == 208 && kAgentWords == 2 + 3 * PO_AGENT_MAX_PTS, "po_agent is read and written as 26 words");

__device__ __forceinline__ double ag_min(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ double ag_max(double a, double b) { return b > a ? b : a; }
__device__ __forceinline__ bool ag_finite(double v) { return fabs(v) <= DBL_MAX; }  // false for NaN and +-inf
__device__ __forceinline__ int ag_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// A record G held as kAgentWords doubles
__device__ __forceinline__ int agent_np(const double *G) { return (int)(unsigned)(__double_as_longlong(G[0]) & 0xffffffffll); }
__device__ __forceinline__ int agent_flags(const double *G) { return (int)(__double_as_longlong(G[0]) >> 32); }
__device__ __forceinline__ double agent_R(const double *G) { return G[1]; }
__device__ __forceinline__ const double *agent_T(const double *G) { return G + 2; }
__device__ __forceinline__ const double *agent_X(const double *G) { return G + 2 + PO_AGENT_MAX_PTS; }
__device__ __forceinline__ const double *agent_Y(const double *G) { return G + 2 + 2 * PO_AGENT_MAX_PTS; }

// The agents [lo, hi) of path b's set: the device entries cannot refuse a table they cannot read, so everything is clamped
__device__ __forceinline__ void agent_set_range(const int *first, const int *set_of, int b, int S, int n_agents, int &lo, int &hi) {
    const int k = ag_clamp(set_of ? set_of[b] : 0, S - 1);
    lo = ag_clamp(first[k], n_agents);
    hi = ag_clamp(first[k + 1], n_agents);
}

struct AgentKeepAll {
    __device__ bool operator()(const double *, int) const { return true; }
};
// The workgroup (kThreads threads, all of them here) copies cnt <= kAgentChunk records to ag_l, and thread j judges agent j: np_l[j] is its number of points, or 0
// when it covers nothing (or when `keep`, asked only about an agent that covers something, drops it).  Three barriers: the first one ends the reads of the previous
// chunk and publishes what the caller wrote to LDS before.
template <int kThreads, class Keep = AgentKeepAll>
__device__ __forceinline__ void agent_chunk_load(const po_agent *agents, int cnt, double *ag_l, int *np_l, Keep keep = Keep{}) {
    const int tid = threadIdx.x;
    __syncthreads();
    const double *src = reinterpret_cast<const double *>(agents);
    for (int w = tid; w < cnt * kAgentWords; w += kThreads) ag_l[w] = src[w];
    __syncthreads();
    if (tid < cnt) {
        const double *G = ag_l + tid * kAgentWords, *T = agent_T(G), *X = agent_X(G), *Y = agent_Y(G);
        const int np = agent_np(G);
        bool covers = np >= 1 && np <= PO_AGENT_MAX_PTS && agent_R(G) >= 0;
        for (int j = 0; j < PO_AGENT_MAX_PTS; ++j)
            if (covers && j < np) covers = ag_finite(T[j]) && ag_finite(X[j]) && ag_finite(Y[j]);
        np_l[tid] = covers && keep(G, np) ? np : 0;
    }
    __syncthreads();
}

// The pieces of the agent at G (np points, judged by agent_chunk_load) over the window [w0, w1], in the definition's order: p = -1 the hold before, 0 .. np - 2
// segment p, np - 1 the hold after.  f(ta, tb, axa, aya, axb, ayb) gets the times the piece is clipped to and the agent's centre at both.  f is called from each
// of the three branches, not once behind them: the compiler then keeps a body of its own for the holds, where the agent stands still, and every kernel needs no
// more registers per wave slot than with the walk written out in it (one call behind the branches cost po_nudge.hip two VGPRs and a wave per SIMD).
template <class F>
__device__ __forceinline__ void agent_pieces(const double *G, int np, double w0, double w1, F f) {
    const double *T = agent_T(G), *X = agent_X(G), *Y = agent_Y(G);
    const int flags = agent_flags(G);
    for (int p = -1; p < np; ++p) {
        if (p < 0) {
            if (!(flags & PO_AGENT_HOLD_BEFORE)) continue;
            const double ta = w0, tb = ag_min(w1, T[0]);
            if (!(ta <= tb)) continue;
            f(ta, tb, X[0], Y[0], X[0], Y[0]);
        } else if (p == np - 1) {
            if (!(flags & PO_AGENT_HOLD_AFTER)) continue;
            const double ta = ag_max(w0, T[p]), tb = w1;
            if (!(ta <= tb)) continue;
            f(ta, tb, X[p], Y[p], X[p], Y[p]);
        } else {
            const double D = T[p + 1] - T[p];
            if (!(D > 0)) continue;
            const double ta = ag_max(w0, T[p]), tb = ag_min(w1, T[p + 1]);
            if (!(ta <= tb)) continue;
            const double wa = (ta - T[p]) / D, wb = (tb - T[p]) / D;
            const double DX = X[p + 1] - X[p], DY = Y[p + 1] - Y[p];
            f(ta, tb, X[p] + wa * DX, Y[p] + wa * DY, X[p] + wb * DX, Y[p] + wb * DY);
        }
    }
}

// A circle of radius cr against an agent of radius R: the circle's centre relative to the agent's goes from (rax, ray) to (rbx, rby); the closest approach
__device__ __forceinline__ double agent_gap(double rax, double ray, double rbx, double rby, double cr, double R) {
    const double dx = rbx - rax, dy = rby - ray, px = -rax, py = -ray;
    const double L2 = dx * dx + dy * dy, dot = px * dx + py * dy;
    double u = L2 > 0 ? dot / L2 : 0;
    u = u < 0 ? 0 : u;
    u = u > 1 ? 1 : u;
    const double qx = px - u * dx, qy = py - u * dy;
    return (sqrt(qx * qx + qy * qy) - cr) - R;
}

}  // namespace po
