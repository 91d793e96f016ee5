// po_dynamic.hip — moving obstacles: B timed paths against per-instance sets of agents on piecewise-linear predicted trajectories, the
// continuous-time closest approach of the six footprint circles to every agent, the first conflict and the v_limit rows that make po_speed_batch* stop short of it.
// The definition is the comment at po_dynamic_batch in include/po_hip.h; this file matches it bit for bit, so it is compiled with -ffp-contract=off (see Makefile)
// and every expression below keeps the order the definition writes.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "../../include/po_hip.h"
#include "../../include/po_pmath.h"
#include "po_launch.hpp"
#include "po_map.hpp"

namespace po {

// (tests/test_dynamic.py places its agent counts around this: DYN_CHUNK there repeats it and changes with it)
constexpr int kDynChunk = 32;                       // agents per LDS chunk
constexpr int kAgentWords = sizeof(po_agent) / 8;   // an agent as 8-byte words: (n_pts, flags), radius, t[8], x[8], y[8]
static_assert(sizeof(po_agent) == 208 && kAgentWords == 2 + 3 * PO_AGENT_MAX_PTS, "po_agent is read as 26 words");

__device__ __forceinline__ double dyn_min(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ double dyn_max(double a, double b) { return b > a ? b : a; }
__device__ __forceinline__ bool dyn_finite(double v) { return fabs(v) <= DBL_MAX; }  // false for NaN and +-inf
__device__ __forceinline__ int dyn_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// One wave per path, lanes over intervals, 64 intervals a tile.  A lane holds the six circle centres of its interval's first state and their differences to the
// second one in registers (the circle loop is unrolled for that: a register array indexed by a loop counter would go to scratch) and walks the agents of the
// path's set, which the wave moves through LDS kDynChunk at a time: every lane reads the same agent word, a broadcast.  A set that fits one chunk is loaded once,
// a longer one once per tile.  The wave is the whole workgroup, so every barrier below is reached by all of it: the loops around them have wave-uniform bounds.
__global__ __launch_bounds__(64) void dynamic_check_kernel(DevCar c, DevDynamic a) {
    __shared__ double ag_l[kDynChunk * kAgentWords];
    __shared__ int np_l[kDynChunk];  // points of the agent; 0: it covers nothing
    const int b = blockIdx.x, lane = threadIdx.x, N = a.N;
    const int n = dyn_clamp(a.n_states ? a.n_states[b] : N, N);
    const double *st = a.states + (size_t)b * N * 5, *tr = a.t + (size_t)b * N;
    const double *lin = a.v_limit_in ? a.v_limit_in + (size_t)b * N : nullptr;
    double *grow = a.gap ? a.gap + (size_t)b * N : nullptr, *lrow = a.v_limit ? a.v_limit + (size_t)b * N : nullptr;

    const bool good = (a.ok ? a.ok[b] != 0 : true) && n >= 2;  // wave-uniform
    bool finite = true;
    if (good)
        for (int i = lane; i < n; i += 64) {
            const double *r = st + 5 * (size_t)i;
            finite = finite && dyn_finite(r[0]) && dyn_finite(r[1]) && dyn_finite(r[2]) && dyn_finite(tr[i]);
        }
    const bool checked = good && !__any(!finite);

    double gmin = DBL_MAX;
    int fi = INT_MAX, fa = -1;  // the first interval of this lane below the margin, and its agent
    if (checked) {
        const int k = dyn_clamp(a.set_of ? a.set_of[b] : 0, a.S - 1);
        const int lo = dyn_clamp(a.first[k], a.n_agents), hi = dyn_clamp(a.first[k + 1], a.n_agents);
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
            for (int c0 = lo; c0 < hi; c0 += kDynChunk) {
                const int cnt = (hi - c0) < kDynChunk ? (hi - c0) : kDynChunk;
                if (t0 == 0 || hi - lo > kDynChunk) {  // (wave-uniform)
                    __syncthreads();
                    const double *src = reinterpret_cast<const double *>(a.agents + c0);
                    for (int w = lane; w < cnt * kAgentWords; w += 64) ag_l[w] = src[w];
                    __syncthreads();
                    if (lane < cnt) {  // lane j judges agent j of the chunk
                        const double *A = ag_l + lane * kAgentWords;
                        int np = (int)(unsigned)(__double_as_longlong(A[0]) & 0xffffffffll);
                        bool covers = np >= 1 && np <= PO_AGENT_MAX_PTS && A[1] >= 0;
                        for (int j = 0; j < PO_AGENT_MAX_PTS; ++j)
                            if (covers && j < np) covers = dyn_finite(A[2 + j]) && dyn_finite(A[10 + j]) && dyn_finite(A[18 + j]);
                        np_l[lane] = covers ? np : 0;
                    }
                    __syncthreads();
                }
                if (!act) continue;
                for (int j = 0; j < cnt; ++j) {
                    const int np = np_l[j];
                    if (np == 0) continue;
                    const double *A = ag_l + j * kAgentWords, *T = A + 2, *X = A + 2 + PO_AGENT_MAX_PTS, *Y = A + 2 + 2 * PO_AGENT_MAX_PTS;
                    const int flags = (int)(__double_as_longlong(A[0]) >> 32);
                    const double R = A[1];
                    for (int p = -1; p < np; ++p) {  // p = -1: before; 0 .. np - 2: segment p; np - 1: after   (wave-uniform)
                        double ta, tb, axa, aya, axb, ayb;
                        if (p < 0) {
                            if (!(flags & PO_AGENT_HOLD_BEFORE)) continue;
                            ta = t_i; tb = dyn_min(t_n, T[0]);
                            if (!(ta <= tb)) continue;
                            axa = axb = X[0]; aya = ayb = Y[0];
                        } else if (p == np - 1) {
                            if (!(flags & PO_AGENT_HOLD_AFTER)) continue;
                            ta = dyn_max(t_i, T[p]); tb = t_n;
                            if (!(ta <= tb)) continue;
                            axa = axb = X[p]; aya = ayb = Y[p];
                        } else {
                            const double D = T[p + 1] - T[p];
                            if (!(D > 0)) continue;
                            ta = dyn_max(t_i, T[p]); tb = dyn_min(t_n, T[p + 1]);
                            if (!(ta <= tb)) continue;
                            const double wa = (ta - T[p]) / D, wb = (tb - T[p]) / D;
                            const double DX = X[p + 1] - X[p], DY = Y[p + 1] - Y[p];
                            axa = X[p] + wa * DX; aya = Y[p] + wa * DY;
                            axb = X[p] + wb * DX; ayb = Y[p] + wb * DY;
                        }
                        const double ua = (ta - t_i) / dt, ub = (tb - t_i) / dt;
#pragma unroll
                        for (int q = 0; q < 6; ++q) {
                            const double rax = (gx[q] + ua * ex[q]) - axa, ray = (gy[q] + ua * ey[q]) - aya;
                            const double rbx = (gx[q] + ub * ex[q]) - axb, rby = (gy[q] + ub * ey[q]) - ayb;
                            const double dx = rbx - rax, dy = rby - ray, px = -rax, py = -ray;
                            const double L2 = dx * dx + dy * dy, dot = px * dx + py * dy;
                            double u = L2 > 0 ? dot / L2 : 0;
                            u = u < 0 ? 0 : u;
                            u = u > 1 ? 1 : u;
                            const double qx = px - u * dx, qy = py - u * dy;
                            const double gap = (sqrt(qx * qx + qy * qy) - c.cr[q]) - R;
                            if (gap < g) { g = gap; arg = c0 + j; }
                        }
                    }
                }
            }
            if (in_path) {
                if (grow) grow[i] = g;
                gmin = dyn_min(gmin, g);
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
        gmin = dyn_min(gmin, __shfl_xor(gmin, h));
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
