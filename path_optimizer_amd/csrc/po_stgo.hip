// po_stgo.hip — station-time plans that resume, sampled in time: the search of po_stplan.hip with the rule "a stopped vehicle stays stopped"
// taken out (po_stsearch.hpp, kResume = true), and the chosen plan sampled at Q uniform time steps in the layouts of po_trajectory_out: drive, stop, wait, go.
// The definition is the comment at po_stgo_batch in include/po_hip.h; this file matches it bit for bit, so it is compiled with -ffp-contract=off (see Makefile)
// and every expression below keeps the order the definition writes.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "po_launch.hpp"
#include "po_stsearch.hpp"

namespace po {

// What the sampler adds to the static LDS: V_k and A_k of the plan.  (The first held sample of every wave goes through StShared::np, the point counts of the
// last agent chunk, which nobody reads after phase 1.)
struct StgoShared {
    double V[PO_ST_MAX_LAYERS + 1], Acc[PO_ST_MAX_LAYERS + 1];
};
static_assert(sizeof(StgoShared) <= 2 * (PO_ST_MAX_LAYERS + 1) * sizeof(double), "the sampler's LDS: 2 * (layers + 1) doubles");
static_assert(kStThreads / 64 <= kAgentChunk, "one slot of StShared::np per wave");
static_assert(stp_lds_bytes(PO_ST_MAX_LAYERS, PO_ST_MAX_STATIONS, PO_ST_MAX_STEP) + sizeof(StShared) + sizeof(StgoShared) <= kLdsLimit, "stgo_kernel's LDS at the limits");

// The sample rows of a path without a plan (not planned, or no plan): zeros, index -1, first_held -1, end 0, n_resumes 0
__device__ __forceinline__ void stgo_no_samples(const DevStgo &a, int b) {
    const int tid = threadIdx.x, Q = a.Q;
    double *o_st = a.o_states + (size_t)b * Q * 5;
    for (int q = tid; q < Q; q += kStThreads) {
        double *w = o_st + 5 * (size_t)q;
        w[0] = 0.0; w[1] = 0.0; w[2] = 0.0; w[3] = 0.0; w[4] = 0.0;
        if (a.o_v) a.o_v[(size_t)b * Q + q] = 0.0;
        if (a.o_a) a.o_a[(size_t)b * Q + q] = 0.0;
        if (a.o_t) a.o_t[(size_t)b * Q + q] = 0.0;
        if (a.index) a.index[(size_t)b * Q + q] = -1;
    }
    if (tid == 0) {
        if (a.n_resumes) a.n_resumes[b] = 0;
        if (a.first_held) a.first_held[b] = -1;
        if (a.end) a.end[b] = 0;
    }
}

// One workgroup per path: the phases of po_stsearch.hpp, then the sampler while the plan, S and V are in LDS.  Lanes over the Q samples: each finds its window,
// bisects the path's s row in global memory between the two stations of its edge and writes its rows.  first_held is an integer minimum over the workgroup.
// Every barrier is reached by the whole workgroup: the early returns are uniform.
__global__ __launch_bounds__(kStThreads) void stgo_kernel(DevCar c, DevStgo a) {
    extern __shared__ double stgo_lds[];
    __shared__ StShared sh;
    __shared__ StgoShared sg;
    const int tid = threadIdx.x, Q = a.Q, stride = a.stride;
    StPath p;
    if (!st_begin<true>(a, sh, stgo_lds, p)) {  // (uniform)
        st_not_planned(a, p);
        stgo_no_samples(a, p.b);
        return;
    }
    st_stations(c, a, p);
    const int blocked = st_blocked(c, a, sh, p);
    const int nl = st_search<true>(a, sh, p);
    st_plan_out(a, sh, p, nl, blocked);
    if (nl == 0) {  // (uniform)
        stgo_no_samples(a, p.b);
        return;
    }

    // ---- the plan's speeds: V_0 = v0, V_k = v(station[k], u_k), A_k = (V_k - V_{k-1}) / dt ----
    const double dt = a.dt;
    if (tid <= nl) {
        const double Vk = tid == 0 ? p.v0 : (p.S[sh.st[tid]] - p.S[sh.st[tid] - sh.u[tid]]) / dt;
        sg.V[tid] = Vk;
        if (tid >= 1) {
            const double Vp = tid == 1 ? p.v0 : (p.S[sh.st[tid - 1]] - p.S[sh.st[tid - 1] - sh.u[tid - 1]]) / dt;
            sg.Acc[tid] = (Vk - Vp) / dt;
        }
    }
    __syncthreads();

    // ---- the samples ----
    const int b = p.b;
    double *o_st = a.o_states + (size_t)b * Q * 5;
    double *o_v = a.o_v ? a.o_v + (size_t)b * Q : nullptr, *o_a = a.o_a ? a.o_a + (size_t)b * Q : nullptr, *o_t = a.o_t ? a.o_t + (size_t)b * Q : nullptr;
    int *o_idx = a.index ? a.index + (size_t)b * Q : nullptr;
    int fh = Q;
    for (int q = tid; q < Q; q += kStThreads) {
        const double T = a.t0 + (double)q * a.dts;
        double x, y, z, kap, s, v, acc;
        int index;
        int row = -1;  // >= 0: the sample is that state's row
        if (T < 0) {
            row = 0; v = p.v0; acc = 0.0;
        } else {
            int kk = 0;
            for (int k = 1; k <= nl; ++k)
                if ((double)k * dt <= T) kk = k;  // (double)k * dt is non-decreasing in k
            if (kk == nl) {  // held
                row = sh.st[nl] * stride; v = sg.V[nl]; acc = 0.0;
                fh = q < fh ? q : fh;
            } else {
                const int ps = sh.st[kk], js = sh.st[kk + 1];
                const double tau = T - (double)kk * dt;
                if (js == ps) {  // standing
                    row = ps * stride; v = 0.0; acc = sg.Acc[kk + 1];
                } else {  // moving: the largest state i of the edge with s_i <= sx (s is non-decreasing: any search finds the same i)
                    const double Vk = sg.V[kk + 1], Sj = p.S[js];
                    const double sig = Vk * tau;
                    double sx = p.S[ps] + sig;
                    sx = sx > Sj ? Sj : sx;
                    int lo = ps * stride, hi = js * stride;  // s_lo <= sx throughout; every index read lies in [lo, hi - 1], hi <= n - 1
                    while (hi - lo > 1) {
                        const int mid = lo + ((hi - lo) >> 1);
                        if (p.st[5 * (size_t)mid + 4] <= sx) lo = mid; else hi = mid;
                    }
                    const int i = lo;
                    const double *r = p.st + 5 * (size_t)i;
                    const double ds = r[9] - r[4];
                    double lam = ds > 0 ? (sx - r[4]) / ds : 0;
                    lam = lam < 0 ? 0 : lam;
                    lam = lam > 1 ? 1 : lam;
                    x = r[0] + lam * (r[5] - r[0]);
                    y = r[1] + lam * (r[6] - r[1]);
                    kap = r[3] + lam * (r[8] - r[3]);
                    s = r[4] + lam * ds;
                    double dz = r[7] - r[2];
                    if (dz > 3.141592653589793) dz = dz - 6.283185307179586;
                    else if (dz < -3.141592653589793) dz = dz + 6.283185307179586;
                    z = r[2] + lam * dz;
                    v = Vk; acc = sg.Acc[kk + 1]; index = i;
                }
            }
        }
        if (row >= 0) {
            const double *r = p.st + 5 * (size_t)row;
            x = r[0]; y = r[1]; z = r[2]; kap = r[3]; s = r[4]; index = row;
        }
        double *w = o_st + 5 * (size_t)q;
        w[0] = x; w[1] = y; w[2] = z; w[3] = kap; w[4] = s;
        if (o_v) o_v[q] = v;
        if (o_a) o_a[q] = acc;
        if (o_t) o_t[q] = T;
        if (o_idx) o_idx[q] = index;
    }
    for (int h = 32; h > 0; h >>= 1) {
        const int o = __shfl_xor(fh, h);
        fh = o < fh ? o : fh;
    }
    if ((tid & 63) == 0) sh.np[tid >> 6] = fh;  // (the barriers of the search lie between phase 1's last read of np and this write)
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kStThreads / 64; ++w) fh = sh.np[w] < fh ? sh.np[w] : fh;
        int nres = 0;
        for (int k = 2; k <= nl; ++k) nres += (sh.u[k - 1] == 0 && sh.u[k] > 0) ? 1 : 0;
        if (a.n_resumes) a.n_resumes[b] = nres;
        if (a.first_held) a.first_held[b] = fh;
        if (a.end) a.end[b] = fh == Q ? 1 : (sh.st[nl] == p.M - 1 ? 2 : (sh.u[nl] == 0 ? 3 : 4));
    }
}

}  // namespace po

extern "C" hipError_t po_launch_stgo(const po::DevCar *c, const po::DevStgo *a, hipStream_t st) {
    const size_t lds = po::stp_lds_bytes(a->K, a->Mb, a->U);
    if (lds + sizeof(po::StShared) + sizeof(po::StgoShared) > po::kLdsLimit) return hipErrorInvalidValue;  // (the entry's ranges keep it below: the static_assert above)
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&po::stgo_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(po::stgo_kernel, dim3(a->B), dim3(po::kStThreads), lds, st, *c, *a);
    return hipGetLastError();
}
