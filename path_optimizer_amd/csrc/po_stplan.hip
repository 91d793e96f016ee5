// po_stplan.hip — station-time speed planning: per path, the (time window, station) cells the agents of its set block, then a layered
// shortest-path search over (station, stations advanced in the last step) that passes ahead of an agent, eases off behind it or stops, and the v_limit rows that
// hand the plan to po_speed_batch*.  The definition is the comment at po_stplan_batch in include/po_hip.h; this file matches it bit for bit, so it is compiled with
// -ffp-contract=off (see Makefile) and every expression below keeps the order the definition writes.  What it shares with the other readers of agents (the chunk
// through LDS, the walk over an agent's pieces, the closest approach) is po_agents.hpp's; the phases of the search are po_stsearch.hpp's, which po_stgo.hip (plans
// that resume after a stop, sampled in time) instantiates with kResume = true.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "po_launch.hpp"
#include "po_stsearch.hpp"

namespace po {

// One workgroup per path: the phases of po_stsearch.hpp (stations, blocked cells, the search with kResume = false: a vehicle that has stopped stays stopped, the
// back-trace), then the v_limit rows.  Every barrier is reached by the whole workgroup: the loops around them have workgroup-uniform bounds, and the early return
// of a path that is not planned is uniform too.
__global__ __launch_bounds__(kStThreads) void stplan_kernel(DevCar c, DevStplan a) {
    extern __shared__ double stp_lds[];
    __shared__ StShared sh;
    const int tid = threadIdx.x, N = a.N, stride = a.stride;
    StPath p;
    const bool planned = st_begin<false>(a, sh, stp_lds, p);
    const int n = p.n;
    const double *lin = a.v_limit_in ? a.v_limit_in + (size_t)p.b * N : nullptr;
    double *lrow = a.v_limit ? a.v_limit + (size_t)p.b * N : nullptr;
    const double dt = a.dt;

    if (!planned) {  // (uniform)
        if (lrow)
            for (int i = tid; i < N; i += kStThreads) lrow[i] = lin ? lin[i] : -1.0;
        st_not_planned(a, p);
        return;
    }
    st_stations(c, a, p);
    const int blocked = st_blocked(c, a, sh, p);
    const int nl = st_search<false>(a, sh, p);
    const double *S_l = p.S;
    const int *plan_st = sh.st, *plan_u = sh.u;
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
    st_plan_out(a, sh, p, nl, blocked);
}

}  // namespace po

extern "C" hipError_t po_launch_stplan(const po::DevCar *c, const po::DevStplan *a, hipStream_t st) {
    const size_t lds = po::stp_lds_bytes(a->K, a->Mb, a->U);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&po::stplan_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(po::stplan_kernel, dim3(a->B), dim3(po::kStThreads), lds, st, *c, *a);
    return hipGetLastError();
}
