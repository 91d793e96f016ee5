// po_agentsets.hip — agent sets: for each of B ego paths, the records of its pool of the two source lists that are not its own and that
// come near the path in space and in time, copied into one array in the po_agent_lists layout po_dynamic.hip, po_stplan.hip and po_nudge.hip read.  The
// definition is the comment at po_agentsets_batch in include/po_hip.h; this file matches it bit for bit, so it is compiled with -ffp-contract=off (see Makefile)
// and every expression below keeps the order the definition writes.  Three launches: count (one wave per ego), scan (one workgroup), gather (one wave per ego).
// No atomics and no scratch: out->count and out->first carry the counts and the offsets from one launch to the next.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

#include "../../include/po_hip.h"
#include "po_agents.hpp"
#include "po_launch.hpp"
#include "po_map.hpp"

namespace po {

// (tests/test_agentsets.py places its batch sizes around this: it reads the constant from here)
constexpr int kSetsScanChunk = 1024;  // egos per step of the scan: the threads of its one workgroup
static_assert(kSetsScanChunk % 64 == 0 && kSetsScanChunk <= 1024, "whole waves, one workgroup");

// What ego b asks of a record: whether it is composed at all, its path's box and its time span.  Wave-uniform after sets_ego.
struct SetsEgo {
    bool composed;
    double exl, exh, eyl, eyh, W0, W1;
};

__device__ __forceinline__ double sets_wave_min(double v) {
    for (int h = 32; h > 0; h >>= 1) v = ag_min(v, __shfl_xor(v, h));
    return v;
}
__device__ __forceinline__ double sets_wave_max(double v) {
    for (int h = 32; h > 0; h >>= 1) v = ag_max(v, __shfl_xor(v, h));
    return v;
}

// One wave: lanes over the rows < n of ego b — the status-0 test by a ballot, the box and the span by shuffle reductions (minima and maxima of finite values:
// any order gives the same value, and the sign of a zero cannot show in a comparison).
__device__ __forceinline__ SetsEgo sets_ego(const DevAgentSets &a, int b, int lane) {
    SetsEgo e;
    const int N = a.N, n = ag_clamp(a.n_states ? a.n_states[b] : N, N);
    const double *st = a.states + (size_t)b * N * 5, *tr = a.t ? a.t + (size_t)b * N : nullptr;
    const bool good = (a.ok ? a.ok[b] != 0 : true) && n >= 1;  // wave-uniform
    bool bad = false;
    double xl = INFINITY, xh = -INFINITY, yl = INFINITY, yh = -INFINITY, tl = INFINITY, th = -INFINITY;
    if (good)
        for (int i = lane; i < n; i += 64) {
            const double x = st[5 * (size_t)i], y = st[5 * (size_t)i + 1];
            bad = bad || !(ag_finite(x) && ag_finite(y));
            xl = ag_min(xl, x); xh = ag_max(xh, x); yl = ag_min(yl, y); yh = ag_max(yh, y);
            if (tr) {
                const double t = tr[i];
                bad = bad || !ag_finite(t);
                tl = ag_min(tl, t); th = ag_max(th, t);
            }
        }
    e.composed = good && !__any(bad);
    e.exl = sets_wave_min(xl); e.exh = sets_wave_max(xh); e.eyl = sets_wave_min(yl); e.eyh = sets_wave_max(yh);
    if (tr) {
        e.W0 = sets_wave_min(tl) - a.t_before;
        e.W1 = sets_wave_max(th) + a.t_after;
    } else {
        e.W0 = a.win_lo; e.W1 = a.win_hi;
    }
    return e;
}

// The pool [lo, hi) of source s that ego b draws from: agent_set_range with pool_of in the place of set_of (everything clamped).  Source 1 may be absent.
__device__ __forceinline__ void sets_pool(const DevAgentSets &a, int s, int b, int &lo, int &hi) {
    lo = hi = 0;
    if (a.S[s] >= 1 && a.n_agents[s] >= 1) agent_set_range(a.first[s], a.pool_of, b, a.S[s], a.n_agents[s], lo, hi);
}

// Is record idx of source s kept for ego b?  The conjunction of the definition's four tests; they have no side effects, so the cheap ones go first and a record
// that fails one is not read further.  Both the count and the gather kernel decide through this function.
__device__ __forceinline__ bool sets_keep(const DevAgentSets &a, const SetsEgo &e, int b, int s, int idx) {
    if (s == 0) {
        if (a.owner) {
            if (a.owner[idx] == b) return false;
        } else if (a.owner_div > 0 && idx / a.owner_div == b) {
            return false;
        }
    }
    const double *G = reinterpret_cast<const double *>(a.agents[s] + idx);
    const int np = agent_np(G), flags = agent_flags(G);
    const double R = agent_R(G);
    if (!(np >= 1 && np <= PO_AGENT_MAX_PTS && R >= 0)) return false;
    const double *T = agent_T(G), *X = agent_X(G), *Y = agent_Y(G);
    bool fin = true;
    double A0 = INFINITY, A1 = -INFINITY;
#pragma unroll
    for (int j = 0; j < PO_AGENT_MAX_PTS; ++j)
        if (j < np) {
            const double t = T[j];
            fin = fin && ag_finite(t);
            A0 = ag_min(A0, t); A1 = ag_max(A1, t);
        }
    if (flags & PO_AGENT_HOLD_BEFORE) A0 = -INFINITY;
    if (flags & PO_AGENT_HOLD_AFTER) A1 = INFINITY;
    if (!(fin && A0 <= e.W1 && A1 >= e.W0)) return false;
    double axl = INFINITY, axh = -INFINITY, ayl = INFINITY, ayh = -INFINITY;
#pragma unroll
    for (int j = 0; j < PO_AGENT_MAX_PTS; ++j)
        if (j < np) {
            const double x = X[j], y = Y[j];
            fin = fin && ag_finite(x) && ag_finite(y);
            axl = ag_min(axl, x); axh = ag_max(axh, x); ayl = ag_min(ayl, y); ayh = ag_max(ayh, y);
        }
    const double rr = R + a.reach;
    return fin && axl - rr <= e.exh && axh + rr >= e.exl && ayl - rr <= e.eyh && ayh + rr >= e.eyl;
}

// One wave per ego: the rows, then the candidates 64 at a time, one record per lane.  count[b], and status[b] as 0 / 1 (the scan makes a clipped 1 a 2).
__global__ __launch_bounds__(64) void agentsets_count_kernel(DevAgentSets a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const SetsEgo e = sets_ego(a, b, lane);
    int cnt = 0;
    if (e.composed)
        for (int s = 0; s < PO_SETS_SOURCES; ++s) {
            int lo, hi;
            sets_pool(a, s, b, lo, hi);
            for (long long base = lo; base < hi; base += 64) {  // (64 bits: base + 64 may pass INT_MAX)
                const long long idx = base + lane;
                const bool keep = idx < hi && sets_keep(a, e, b, s, (int)idx);
                cnt += __popcll(__ballot(keep));
            }
        }
    if (lane == 0) {
        a.count[b] = cnt;
        a.status[b] = e.composed ? 1 : 0;
    }
}

// One workgroup: the exclusive scan of count in 64 bits, kSetsScanChunk egos a step with a carry; first (clipped), the clip status, set_of, total.
__global__ __launch_bounds__(kSetsScanChunk) void agentsets_scan_kernel(DevAgentSets a) {
    constexpr int kWaves = kSetsScanChunk / 64;
    __shared__ long long wsum[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long cap = a.capacity;
    long long carry = 0;
    for (long long base = 0; base < a.B; base += kSetsScanChunk) {
        const long long bb = base + tid;
        const bool live = bb < a.B;
        const int b = live ? (int)bb : 0;
        const long long c = live ? (long long)a.count[b] : 0;
        long long incl = c;
        for (int d = 1; d < 64; d <<= 1) {
            const long long o = __shfl_up(incl, d);
            if (lane >= d) incl += o;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        long long before = 0, all = 0;
        for (int w = 0; w < kWaves; ++w) {
            const long long v = wsum[w];
            before += w < wave ? v : 0;
            all += v;
        }
        if (live) {
            const long long F = carry + before + (incl - c);
            a.o_first[b] = (int)(F < cap ? F : cap);
            if (a.status[b] != 0) a.status[b] = F + c > cap ? 2 : 1;
            if (a.o_set_of) a.o_set_of[b] = b;
        }
        carry += all;
        __syncthreads();  // wsum is rewritten by the next step
    }
    if (tid == 0) {
        a.o_first[a.B] = (int)(carry < cap ? carry : cap);
        if (a.total) a.total[0] = carry;
    }
}

// One wave per ego: the decisions of the count kernel once more; a kept record's rank is the running count plus the kept lanes below it, and the wave copies the
// kept records of a step together, 26 words a record, consecutive lanes to consecutive words of consecutive slots.  An ego whose set starts at or behind the
// capacity writes nothing; a set that crosses it is cut there.
__global__ __launch_bounds__(64) void agentsets_gather_kernel(DevAgentSets a) {
    __shared__ int kept_l[64];  // the record index of the r-th kept lane of the step
    const int b = blockIdx.x, lane = threadIdx.x;
    const int F = a.o_first[b], room = a.capacity - F;  // first[b] == F_b wherever F_b < capacity
    const int want = a.count[b] < room ? a.count[b] : room;
    if (want <= 0) return;  // wave-uniform: nothing kept, not composed, or clipped away
    const SetsEgo e = sets_ego(a, b, lane);
    const unsigned long long *src_w;
    unsigned long long *dst_w = reinterpret_cast<unsigned long long *>(a.o_agents);
    int done = 0;
    for (int s = 0; s < PO_SETS_SOURCES && done < want; ++s) {
        int lo, hi;
        sets_pool(a, s, b, lo, hi);
        src_w = reinterpret_cast<const unsigned long long *>(a.agents[s]);
        const int tag = s == 0 ? 0 : a.n_agents[0];
        for (long long base = lo; base < hi && done < want; base += 64) {
            const long long idx = base + lane;
            const bool keep = idx < hi && sets_keep(a, e, b, s, (int)idx);
            const unsigned long long mask = __ballot(keep);
            const int r = __popcll(mask & ((1ull << lane) - 1ull));
            int k = __popcll(mask);
            k = k < want - done ? k : want - done;
            __syncthreads();  // the reads of the step before are over
            if (keep && r < k) {
                kept_l[r] = (int)idx;
                if (a.src_index) a.src_index[F + done + r] = tag + (int)idx;
            }
            __syncthreads();
            for (int w = lane; w < k * kAgentWords; w += 64) {
                const int q = w / kAgentWords, word = w - q * kAgentWords;
                dst_w[(size_t)(F + done + q) * kAgentWords + word] = src_w[(size_t)kept_l[q] * kAgentWords + word];
            }
            done += k;
        }
    }
}

}  // namespace po

extern "C" hipError_t po_launch_agentsets(const po::DevAgentSets *a, hipStream_t st) {
    hipLaunchKernelGGL(po::agentsets_count_kernel, dim3(a->B), dim3(64), 0, st, *a);
    hipLaunchKernelGGL(po::agentsets_scan_kernel, dim3(1), dim3(po::kSetsScanChunk), 0, st, *a);
    if (a->capacity > 0) hipLaunchKernelGGL(po::agentsets_gather_kernel, dim3(a->B), dim3(64), 0, st, *a);
    return hipGetLastError();
}
