// po_nudge.hip — corridor nudge: per path, the lateral interval every predicted agent of its set occupies on every (state, covering circle)
// pair of the corridor while the vehicle is expected there, the side the vehicle passes each agent on, and the corridor bounds carved to that side, in the layout
// po_batch_in.bounds reads.  The definition is the comment at po_nudge_batch in include/po_hip.h; this file matches it bit for bit, so it is compiled with
// -ffp-contract=off (see Makefile) and every expression below keeps the order the definition writes.  What it shares with the other readers of agents (the chunk
// through LDS, the walk over an agent's pieces) is po_agents.hpp's.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "../../include/po_hip.h"
#include "../../include/po_pmath.h"
#include "po_agents.hpp"
#include "po_launch.hpp"
#include "po_map.hpp"

namespace po {

// (tests/test_nudge.py places its path lengths around this: NDG_TRIG there repeats it and changes with it)
constexpr int kNdgTrig = 384;  // states whose cos / sin are kept in LDS; the states behind them compute theirs again per agent

__device__ __forceinline__ void ndg_fold(double c, double &lo, double &hi) { lo = ag_min(lo, c); hi = ag_max(hi, c); }

// One piece of an agent, from (axa, aya) to (axb, ayb) in the world, on the pair whose frame is (cx, cy, cz, sz): the candidates of the definition, in its order.
__device__ __forceinline__ void ndg_piece(double axa, double aya, double axb, double ayb, double cx, double cy, double cz, double sz, double rho, double &lo,
                                          double &hi) {
    const double dxa = axa - cx, dya = aya - cy, dxb = axb - cx, dyb = ayb - cy;
    const double ua = dxa * cz + dya * sz, la = (-dxa) * sz + dya * cz;
    const double ub = dxb * cz + dyb * sz, lb = (-dxb) * sz + dyb * cz;
    const double qa = rho * rho - ua * ua;
    if (qa >= 0) {
        const double w = sqrt(qa);
        ndg_fold(la - w, lo, hi);
        ndg_fold(la + w, lo, hi);
    }
    const double qb = rho * rho - ub * ub;
    if (qb >= 0) {
        const double w = sqrt(qb);
        ndg_fold(lb - w, lo, hi);
        ndg_fold(lb + w, lo, hi);
    }
    const double du = ub - ua, dl = lb - la, L2 = du * du + dl * dl;
    if (L2 > 0 && du != 0) {
        const double len = sqrt(L2), ox = (rho * dl) / len, oy = (rho * du) / len;
        const double tp = (ox - ua) / du;
        if (0 <= tp && tp <= 1) ndg_fold((la + oy) + tp * dl, lo, hi);
        const double tm = (0 - (ox + ua)) / du;
        if (0 <= tm && tm <= 1) ndg_fold((la - oy) + tm * dl, lo, hi);
    }
}

// The hull of the agent at G (26 words in LDS, np points) on one pair, over the window [w0, w1] of the pair's state.
__device__ __forceinline__ void ndg_hull(const double *G, int np, double w0, double w1, double cx, double cy, double cz, double sz, double rho, double &lo,
                                         double &hi) {
    lo = DBL_MAX; hi = -DBL_MAX;
    agent_pieces(G, np, w0, w1, [&](double, double, double axa, double aya, double axb, double ayb) { ndg_piece(axa, aya, axb, ayb, cx, cy, cz, sz, rho, lo, hi); });
}

// One wave per path.  Pair p = 4 i + j (state i, circle j) belongs to lane p mod 64, for good: 64 is a multiple of 4, so a lane keeps its circle j = lane & 3 and
// walks the states (lane >> 2) + 16 k.  The working corridor of a lane's pairs lives in out->bounds itself: the lane that wrote a pair is the one that reads it
// again, so nothing needs synchronising, no LDS is sized by N and N has no limit.  The agents of the path's set move through LDS kAgentChunk at a time and are read
// as broadcasts; lane j of the wave judges agent j of the chunk: whether it covers anything, and whether its whole time extent, holds included, meets the path's
// [min t - t_before, max t + t_after] at all — an agent that does not has no live piece on any pair, so skipping it changes no result.  Per live agent: one sweep
// over the lane's pairs for hull and touch, rl, rr and f reduced across the wave; the decision, wave-uniform; and, only when the agent is passed on a side, a
// second sweep that computes the hulls again and moves the bound (most agents touch nothing, so the hulls are not kept).  The wave is the whole workgroup, so every
// barrier below is reached by all of it: the loops around them have wave-uniform bounds.
__global__ __launch_bounds__(64) void nudge_kernel(DevNudge a) {
    __shared__ double ag_l[kAgentChunk * kAgentWords];
    __shared__ int np_l[kAgentChunk];  // points of the agent; 0: it covers nothing, or is nowhere near the path in time
    __shared__ double cz_l[kNdgTrig], sz_l[kNdgTrig];
    const int b = blockIdx.x, lane = threadIdx.x, N = a.N, W = a.W;
    const int n = ag_clamp(a.n_points ? a.n_points[b] : N, N);
    const size_t row = (size_t)b * N;
    const double *X = a.ref_x + row, *Y = a.ref_y + row, *Z = a.ref_z + row, *T = a.t + row, *bin = a.bounds_in + 8 * row;
    double *bo = a.bounds + 8 * row;
    int *srow = a.side ? a.side + (size_t)b * W : nullptr;
    const int *sprev = a.side_prev ? a.side_prev + (size_t)b * W : nullptr;
    const size_t pairs = 4 * (size_t)n, all_pairs = 4 * (size_t)N;

    // every row of the corridor goes to the output first, each pair through the lane that owns it; the rows < n are looked at on the way
    bool finite = true;
    for (size_t p = lane; p < all_pairs; p += 64) {
        const double l = bin[2 * p], u = bin[2 * p + 1];
        bo[2 * p] = l; bo[2 * p + 1] = u;
        if (p < pairs) finite = finite && ag_finite(l) && ag_finite(u);
    }
    for (int i = lane; i < n; i += 64) finite = finite && ag_finite(X[i]) && ag_finite(Y[i]) && ag_finite(Z[i]) && ag_finite(T[i]);
    const bool processed = (a.ok ? a.ok[b] != 0 : true) && n >= 1 && !__any(!finite);  // wave-uniform

    if (!processed) {
        if (srow)
            for (int e = lane; e < W; e += 64) srow[e] = 0;
        if (lane == 0) {
            a.status[b] = 0;
            if (a.ok_out) a.ok_out[b] = 0;
            if (a.first_blocked_state) a.first_blocked_state[b] = -1;
            if (a.first_blocked_agent) a.first_blocked_agent[b] = -1;
            if (a.width_min) a.width_min[b] = DBL_MAX;
        }
        return;
    }

    // the frames' cos / sin of the first kNdgTrig states, and the time extent of the path's windows (minima and maxima of finite values: the order of the
    // butterflies does not change a comparison made with them)
    double tmin = DBL_MAX, tmax = -DBL_MAX;
    for (int i = lane; i < n; i += 64) {
        if (i < kNdgTrig) { cz_l[i] = po_pcos(Z[i]); sz_l[i] = po_psin(Z[i]); }
        tmin = ag_min(tmin, T[i] - a.t_before);
        tmax = ag_max(tmax, T[i] + a.t_after);
    }
    for (int h = 32; h > 0; h >>= 1) {
        tmin = ag_min(tmin, __shfl_xor(tmin, h));
        tmax = ag_max(tmax, __shfl_xor(tmax, h));
    }
    const int jq = lane & 3;
    const double dj = jq == 0 ? a.d[0] : (jq == 1 ? a.d[1] : (jq == 2 ? a.d[2] : a.d[3]));  // (selects: a kernel argument indexed by the lane would go to scratch)
    const size_t p_first = a.skip_states > 0 ? 4 * (size_t)a.skip_states : 0;  // pairs of rows < skip_states are never touched

    int lo_a, hi_a;
    agent_set_range(a.first, a.set_of, b, a.S, a.n_agents, lo_a, hi_a);
    bool carved = false;
    int fb_state = -1, fb_agent = -1;  // the first blocking agent
    for (int c0 = lo_a; c0 < hi_a; c0 += kAgentChunk) {
        const int cnt = (hi_a - c0) < kAgentChunk ? (hi_a - c0) : kAgentChunk;
        // (the load's first barrier: cz_l, sz_l are written; the previous chunk is read)
        agent_chunk_load<64>(a.agents + c0, cnt, ag_l, np_l, [&](const double *G, int np) {  // an agent that covers something: is it near the path in time?
            const double *Ta = agent_T(G);
            const int flags = agent_flags(G);
            double t_lo = DBL_MAX, t_hi = -DBL_MAX;  // every piece lies within [t_lo, t_hi], but for the holds
            for (int j = 0; j < PO_AGENT_MAX_PTS; ++j)
                if (j < np) { t_lo = ag_min(t_lo, Ta[j]); t_hi = ag_max(t_hi, Ta[j]); }
            if (!(flags & PO_AGENT_HOLD_BEFORE) && tmax < t_lo) return false;  // every window ends before the agent appears: tb < ta in every piece
            if (!(flags & PO_AGENT_HOLD_AFTER) && tmin > t_hi) return false;   // every window begins after it is gone
            return true;
        });
        for (int j = 0; j < cnt; ++j) {
            const int np = np_l[j], e = c0 + j - lo_a;
            int side = 0;
            if (np != 0 && p_first < pairs) {  // (wave-uniform)
                const double *G = ag_l + j * kAgentWords;
                const double rho = (a.radius + G[1]) + a.margin;
                double rl = DBL_MAX, rr = DBL_MAX;
                int f = INT_MAX;
                for (size_t p = lane; p < pairs; p += 64) {
                    if (p < p_first) continue;
                    const int i = (int)(p >> 2);
                    const double cz = i < kNdgTrig ? cz_l[i] : po_pcos(Z[i]), sz = i < kNdgTrig ? sz_l[i] : po_psin(Z[i]);
                    double lo, hi;
                    ndg_hull(G, np, T[i] - a.t_before, T[i] + a.t_after, X[i] + dj * cz, Y[i] + dj * sz, cz, sz, rho, lo, hi);
                    const double Wl = bo[2 * p], Wu = bo[2 * p + 1];
                    if (lo <= hi && hi > Wl && lo < Wu) {
                        rl = ag_min(rl, Wu - hi);
                        rr = ag_min(rr, lo - Wl);
                        f = i < f ? i : f;
                    }
                }
                for (int h = 32; h > 0; h >>= 1) {  // rl and rr are never NaN
                    rl = ag_min(rl, __shfl_xor(rl, h));
                    rr = ag_min(rr, __shfl_xor(rr, h));
                    const int o = __shfl_xor(f, h);
                    f = o < f ? o : f;
                }
                if (f != INT_MAX) {
                    const bool left = rl >= a.min_width, right = rr >= a.min_width;
                    const int sp = (sprev && e < W) ? sprev[e] : 0;
                    if (sp == 1 && left) side = 1;
                    else if (sp == -1 && right) side = -1;
                    else if (left && right) side = rl >= rr ? 1 : -1;
                    else if (left) side = 1;
                    else if (right) side = -1;
                    else side = 2;
                    if (side == 2) {
                        if (fb_agent < 0) { fb_agent = c0 + j; fb_state = f; }
                    } else {
                        carved = true;
                        for (size_t p = lane; p < pairs; p += 64) {  // the same hulls against the same corridor: the same pairs are touched
                            if (p < p_first) continue;
                            const int i = (int)(p >> 2);
                            const double cz = i < kNdgTrig ? cz_l[i] : po_pcos(Z[i]), sz = i < kNdgTrig ? sz_l[i] : po_psin(Z[i]);
                            double lo, hi;
                            ndg_hull(G, np, T[i] - a.t_before, T[i] + a.t_after, X[i] + dj * cz, Y[i] + dj * sz, cz, sz, rho, lo, hi);
                            const double Wl = bo[2 * p], Wu = bo[2 * p + 1];
                            if (lo <= hi && hi > Wl && lo < Wu) {
                                if (side == 1) bo[2 * p] = hi;
                                else bo[2 * p + 1] = lo;
                            }
                        }
                    }
                }
            }
            if (srow && lane == 0 && e < W) srow[e] = side;
        }
    }
    if (srow)
        for (int e = (hi_a > lo_a ? hi_a - lo_a : 0) + lane; e < W; e += 64) srow[e] = 0;

    double wmin = DBL_MAX;
    for (size_t p = lane; p < pairs; p += 64) {
        double w = bo[2 * p + 1] - bo[2 * p];
        w = w == 0 ? 0.0 : w;  // -0.0 counts as +0.0: the minimum does not depend on the order of the fold
        wmin = ag_min(wmin, w);
    }
    for (int h = 32; h > 0; h >>= 1) wmin = ag_min(wmin, __shfl_xor(wmin, h));
    if (lane == 0) {
        const int status = fb_agent >= 0 ? 3 : (carved ? 2 : 1);
        a.status[b] = status;
        if (a.ok_out) a.ok_out[b] = status != 3 ? 1 : 0;
        if (a.first_blocked_state) a.first_blocked_state[b] = fb_state;
        if (a.first_blocked_agent) a.first_blocked_agent[b] = fb_agent;
        if (a.width_min) a.width_min[b] = wmin;
    }
}

}  // namespace po

extern "C" hipError_t po_launch_nudge(const po::DevNudge *a, hipStream_t st) {
    hipLaunchKernelGGL(po::nudge_kernel, dim3(a->B), dim3(64), 0, st, *a);
    return hipGetLastError();
}
