// po_trajectory.hip — the timed trajectory: B speed-profiled paths sampled at K uniform time steps by the profile's own model (constant
// acceleration per interval), a stop held at the stop state, and the same samples written as po_agent records that the moving-obstacle stages read as they are.
// The definition is the comment at po_trajectory_batch in include/po_hip.h; this file matches it bit for bit, so it is compiled with -ffp-contract=off (see
// Makefile) and every expression below keeps the order the definition writes.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "../../include/po_hip.h"
#include "../../include/po_pmath.h"
#include "po_agents.hpp"  // kAgentWords: a record as 8-byte words
#include "po_launch.hpp"
#include "po_map.hpp"

namespace po {

static_assert(PO_AGENT_MAX_PTS <= 64, "one lane per agent point");

__device__ __forceinline__ bool trj_finite(double v) { return fabs(v) <= DBL_MAX; }  // false for NaN and +-inf
__device__ __forceinline__ int trj_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

struct TrjSample {
    double x, y, z, k, s, v, a;
    int index;
};

// Sample at time T of a SAMPLED path (rows < n validated, E and tE = t_E from the sweep): held at row E, before the path at row 0, or inside interval i found by
// bisection on the t row with t_lo <= T < t_hi kept throughout ([0, E] to start with: T >= t_0 and T < t_E here).  t is non-decreasing, so the largest i with
// t_i <= T is what any search finds.  Every index read lies in [0, E], E <= n - 1.
__device__ __forceinline__ TrjSample trj_sample(const double *st, const double *vr, const double *tr, int E, double tE, double T) {
    TrjSample o;
    int row = -1;
    if (T >= tE) row = E;
    else if (T < tr[0]) row = 0;
    if (row >= 0) {
        const double *r = st + 5 * (size_t)row;
        o.x = r[0]; o.y = r[1]; o.z = r[2]; o.k = r[3]; o.s = r[4];
        o.v = vr[row]; o.a = 0.0; o.index = row;
        return o;
    }
    int lo = 0, hi = E;
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (tr[mid] <= T) lo = mid; else hi = mid;
    }
    const int i = lo;
    const double *r = st + 5 * (size_t)i;
    const double t_i = tr[i], v_i = vr[i];
    const double Dt = tr[i + 1] - t_i;
    const double tau = T - t_i;
    const double acc = (vr[i + 1] - v_i) / Dt;
    const double sig = (v_i + (0.5 * acc) * tau) * tau;
    const double ds = r[9] - r[4];
    double lam = ds > 0 ? sig / ds : 0;
    lam = lam < 0 ? 0 : lam;
    lam = lam > 1 ? 1 : lam;
    o.x = r[0] + lam * (r[5] - r[0]);
    o.y = r[1] + lam * (r[6] - r[1]);
    o.k = r[3] + lam * (r[8] - r[3]);
    o.s = r[4] + lam * ds;
    double dz = r[7] - r[2];
    if (dz > 3.141592653589793) dz = dz - 6.283185307179586;
    else if (dz < -3.141592653589793) dz = dz + 6.283185307179586;
    o.z = r[2] + lam * dz;
    const double vv = v_i + acc * tau;
    o.v = vv > 0 ? vv : 0;
    o.a = acc;
    o.index = i;
    return o;
}

// One wave per path.  Sweep 1, lanes over the rows: the status-0 test and the end state E, a ballot and an integer minimum (any order gives the same result).
// Sweep 2, lanes over the samples: each lane computes T, bisects and writes its sample's row of every output asked for.  The agent records: lane j < 8 owns
// point j of all D records of the path (it samples k = j * stride once more rather than wait for the lane that owns k), lane 0 also their headers; the words of
// the points >= P are zeros from their lanes.  No LDS, no barrier: nothing is shared but the two reductions.
__global__ __launch_bounds__(64) void trajectory_kernel(DevTrajectory a) {
    const int b = blockIdx.x, lane = threadIdx.x, N = a.N, K = a.K, D = a.D;
    const int n = trj_clamp(a.n_states ? a.n_states[b] : N, N);
    const double *st = a.states + (size_t)b * N * 5, *vr = a.v + (size_t)b * N, *tr = a.t + (size_t)b * N;
    double *o_st = a.o_states + (size_t)b * K * 5;
    double *o_v = a.o_v ? a.o_v + (size_t)b * K : nullptr, *o_a = a.o_a ? a.o_a + (size_t)b * K : nullptr, *o_t = a.o_t ? a.o_t + (size_t)b * K : nullptr;
    int *o_idx = a.index ? a.index + (size_t)b * K : nullptr;
    po_agent *rec = D > 0 ? a.agents + (size_t)b * D : nullptr;

    const bool good = (a.ok ? a.ok[b] != 0 : true) && n >= 1;  // wave-uniform
    bool bad = false;
    int E = INT_MAX;
    if (good)
        for (int i = lane; i < n; i += 64) {  // ascending: the first rest pair a lane meets is its smallest
            const double *r = st + 5 * (size_t)i;
            const double v_i = vr[i], t_i = tr[i];
            bad = bad || !(trj_finite(r[0]) && trj_finite(r[1]) && trj_finite(r[2]) && trj_finite(r[3]) && trj_finite(r[4]) && trj_finite(v_i) && trj_finite(t_i));
            bad = bad || !(v_i >= 0);
            if (i < n - 1) {
                bad = bad || tr[i + 1] < t_i;
                if (E == INT_MAX && v_i == 0 && vr[i + 1] == 0 && r[9] - r[4] > 0) E = i;
            }
        }
    const bool sampled = good && !__any(bad);
    for (int h = 32; h > 0; h >>= 1) {
        const int o = __shfl_xor(E, h);
        E = o < E ? o : E;
    }

    if (!sampled) {
        for (int k = lane; k < K; k += 64) {
            double *w = o_st + 5 * (size_t)k;
            w[0] = 0.0; w[1] = 0.0; w[2] = 0.0; w[3] = 0.0; w[4] = 0.0;
            if (o_v) o_v[k] = 0.0;
            if (o_a) o_a[k] = 0.0;
            if (o_t) o_t[k] = 0.0;
            if (o_idx) o_idx[k] = -1;
        }
        if (rec) {
            unsigned long long *w = reinterpret_cast<unsigned long long *>(rec);
            for (int i = lane; i < D * kAgentWords; i += 64) w[i] = 0ull;
        }
        if (lane == 0) {
            a.status[b] = 0;
            if (a.first_held) a.first_held[b] = -1;
        }
        return;
    }
    if (E == INT_MAX) E = n - 1;
    const double tE = tr[E];

    int fh = K;
    for (int k = lane; k < K; k += 64) {
        const double T = a.t0 + (double)k * a.dt;
        if (fh == K && T >= tE) fh = k;  // T_k is non-decreasing in k: the first held sample of this lane
        const TrjSample s = trj_sample(st, vr, tr, E, tE, T);
        double *w = o_st + 5 * (size_t)k;
        w[0] = s.x; w[1] = s.y; w[2] = s.z; w[3] = s.k; w[4] = s.s;
        if (o_v) o_v[k] = s.v;
        if (o_a) o_a[k] = s.a;
        if (o_t) o_t[k] = T;
        if (o_idx) o_idx[k] = s.index;
    }
    for (int h = 32; h > 0; h >>= 1) {
        const int o = __shfl_xor(fh, h);
        fh = o < fh ? o : fh;
    }

    if (rec && lane < PO_AGENT_MAX_PTS) {
        const int j = lane;
        const bool live = j < a.P;  // then k = j * stride <= (P - 1) * stride < K: the entry checked it
        double T = 0.0, X = 0.0, Y = 0.0, cz = 0.0, sz = 0.0;
        if (live) {
            T = a.t0 + (double)(j * a.stride) * a.dt;
            const TrjSample s = trj_sample(st, vr, tr, E, tE, T);
            X = s.x; Y = s.y;
            cz = po_pcos(s.z); sz = po_psin(s.z);
        }
#pragma unroll
        for (int d = 0; d < PO_TRAJ_MAX_DISCS; ++d)
            if (d < D) {
                po_agent *g = rec + d;
                g->t[j] = T;
                g->x[j] = live ? X + a.off[d] * cz : 0.0;
                g->y[j] = live ? Y + a.off[d] * sz : 0.0;
                if (j == 0) { g->n_pts = a.P; g->flags = a.flags; g->radius = a.rad[d]; }
            }
    }
    if (lane == 0) {
        a.status[b] = fh == K ? 1 : (vr[E] == 0 ? 2 : 3);
        if (a.first_held) a.first_held[b] = fh;
    }
}

}  // namespace po

extern "C" hipError_t po_launch_trajectory(const po::DevTrajectory *a, hipStream_t st) {
    hipLaunchKernelGGL(po::trajectory_kernel, dim3(a->B), dim3(64), 0, st, *a);
    return hipGetLastError();
}
