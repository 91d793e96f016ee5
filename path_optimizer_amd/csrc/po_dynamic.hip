// po_dynamic.hip — moving obstacles: B timed paths against per-instance sets of agents on piecewise-linear predicted trajectories, the
// continuous-time closest approach of the six footprint circles to every agent, the first conflict and the v_limit rows that make po_speed_batch* stop short of it.
// The definition is the comment at po_dynamic_batch in include/po_hip.h; this file matches it bit for bit, so it is compiled with -ffp-contract=off (see Makefile)
// and every expression below keeps the order the definition writes.  What it shares with the other readers of agents (the chunk through LDS, the walk over an
// agent's pieces, the closest approach) is po_agents.hpp's.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "../../include/po_hip.h"
#include "../../include/po_pmath.h"
#include "po_agents.hpp"
#include "po_launch.hpp"
#include "po_map.hpp"

namespace po {

// One wave per path, lanes over intervals, 64 intervals a tile.  A lane holds the six circle centres of its interval's first state and their differences to the
// second one in registers (the circle loop is unrolled for that: a register array indexed by a loop counter would go to scratch) and walks the agents of the
// path's set, which the wave moves through LDS kAgentChunk at a time: every lane reads the same agent word, a broadcast.  A set that fits one chunk is loaded once,
// a longer one once per tile.  The wave is the whole workgroup, so every barrier below is reached by all of it: the loops around them have wave-uniform bounds.
__global__ __launch_bounds__(64) void dynamic_check_kernel(DevCar c, DevDynamic a) {
    __shared__ double ag_l[kAgentChunk * kAgentWords];
    __shared__ int np_l[kAgentChunk];  // points of the agent; 0: it covers nothing
    const int b = blockIdx.x, lane = threadIdx.x, N = a.N;
    const int n = ag_clamp(a.n_states ? a.n_states[b] : N, N);
    const double *st = a.states + (size_t)b * N * 5, *tr = a.t + (size_t)b * N;
    const double *lin = a.v_limit_in ? a.v_limit_in + (size_t)b * N : nullptr;
    double *grow = a.gap ? a.gap + (size_t)b * N : nullptr, *lrow = a.v_limit ? a.v_limit + (size_t)b * N : nullptr;

    const bool good = (a.ok ? a.ok[b] != 0 : true) && n >= 2;  // wave-uniform
    bool finite = true;
    if (good)
        for (int i = lane; i < n; i += 64) {
            const double *r = st + 5 * (size_t)i;
            finite = finite && ag_finite(r[0]) && ag_finite(r[1]) && ag_finite(r[2]) && ag_finite(tr[i]);
        }
    const bool checked = good && !__any(!finite);

    double gmin = DBL_MAX;
    int fi = INT_MAX, fa = -1;  // the first interval of this lane below the margin, and its agent
    if (checked) {
        int lo, hi;
        agent_set_range(a.first, a.set_of, b, a.S, a.n_agents, lo, hi);
        for (int t0 = 0; t0 < n - 1; t0 += 64) {
            const int i = t0 + lane;
            const bool in_path = i < n - 1;
            double t_i = 0.0, t_n = 0.0, dt = 0.0, gx[6], gy[6], ex[6], ey[6];
            if (in_path) {
                const double *r = st + 5 * (size_t)i;
                t_i = tr[i]; t_n = tr[i + 1];
                dt = t_n - t_i;
                const double cz = po_pcos(r[2]), sz = po_psin(r[2]), cn = po_pcos(r[7]), sn = po_psin(r[7]);
#pragma unroll
                for (int q = 0; q < 6; ++q) {
                    gx[q] = (c.cx[q] * cz - c.cy[q] * sz) + r[0];
                    gy[q] = (c.cx[q] * sz + c.cy[q] * cz) + r[1];
                    ex[q] = ((c.cx[q] * cn - c.cy[q] * sn) + r[5]) - gx[q];
                    ey[q] = ((c.cx[q] * sn + c.cy[q] * cn) + r[6]) - gy[q];
                }
            }
            const bool act = in_path && dt > 0;
            double g = DBL_MAX;
            int arg = -1;
            for (int c0 = lo; c0 < hi; c0 += kAgentChunk) {
                const int cnt = (hi - c0) < kAgentChunk ? (hi - c0) : kAgentChunk;
                if (t0 == 0 || hi - lo > kAgentChunk) agent_chunk_load<64>(a.agents + c0, cnt, ag_l, np_l);  // (wave-uniform)
                if (!act) continue;
                for (int j = 0; j < cnt; ++j) {
                    const int np = np_l[j];
                    if (np == 0) continue;
                    const double *G = ag_l + j * kAgentWords;
                    const double R = agent_R(G);
                    agent_pieces(G, np, t_i, t_n, [&](double ta, double tb, double axa, double aya, double axb, double ayb) {  // (wave-uniform)
                        const double ua = (ta - t_i) / dt, ub = (tb - t_i) / dt;
#pragma unroll
                        for (int q = 0; q < 6; ++q) {
                            const double rax = (gx[q] + ua * ex[q]) - axa, ray = (gy[q] + ua * ey[q]) - aya;
                            const double rbx = (gx[q] + ub * ex[q]) - axb, rby = (gy[q] + ub * ey[q]) - ayb;
                            const double gap = agent_gap(rax, ray, rbx, rby, c.cr[q], R);
                            if (gap < g) { g = gap; arg = c0 + j; }
                        }
                    });
                }
            }
            if (in_path) {
                if (grow) grow[i] = g;
                gmin = ag_min(gmin, g);
                if (fi == INT_MAX && g < a.margin) { fi = i; fa = arg; }
            }
        }
    }
    // the rest of the gap row: every entry for a path that was not checked, entries >= n - 1 otherwise
    if (grow)
        for (int i = (checked ? n - 1 : 0) + lane; i < N; i += 64) grow[i] = DBL_MAX;

    // the wave's verdict: integer minima and maxima and a minimum of doubles that are never NaN and never -0, so the butterflies' order does not matter
    int f = fi;
    for (int h = 32; h > 0; h >>= 1) {
        gmin = ag_min(gmin, __shfl_xor(gmin, h));
        const int o = __shfl_xor(f, h);
        f = o < f ? o : f;
    }
    const bool conflict = f != INT_MAX;
    const int agent = __shfl(fa, conflict ? (f & 63) : 0);  // interval i sits on lane i mod 64 in every tile
    int stop = 0, status = checked ? 1 : 0;
    double t_f = 0.0;
    if (conflict) {
        const double s_stop = st[5 * (size_t)f + 4] - a.stop_distance;
        for (int i = lane; i <= f; i += 64)
            if (st[5 * (size_t)i + 4] <= s_stop) stop = i;  // ascending: the lane's largest
        for (int h = 32; h > 0; h >>= 1) {
            const int o = __shfl_xor(stop, h);
            stop = o > stop ? o : stop;
        }
        status = !(st[4] <= s_stop) ? 3 : 2;
        t_f = tr[f];
    }
    if (lrow)
        for (int i = lane; i < N; i += 64) lrow[i] = (conflict && i >= stop && i < n) ? 0.0 : (lin ? lin[i] : -1.0);
    if (lane == 0) {
        a.status[b] = status;
        if (a.ok_out) a.ok_out[b] = status == 1 ? 1 : 0;
        if (a.gap_min) a.gap_min[b] = gmin;
        if (a.first_state) a.first_state[b] = conflict ? f : -1;
        if (a.first_agent) a.first_agent[b] = conflict ? agent : -1;
        if (a.stop_state) a.stop_state[b] = conflict ? stop : -1;
        if (a.first_time) a.first_time[b] = t_f;
    }
}

}  // namespace po

extern "C" hipError_t po_launch_dynamic(const po::DevCar *c, const po::DevDynamic *a, hipStream_t st) {
    hipLaunchKernelGGL(po::dynamic_check_kernel, dim3(a->B), dim3(64), 0, st, *c, *a);
    return hipGetLastError();
}
