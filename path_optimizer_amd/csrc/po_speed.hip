// po_speed.hip — the speed profile: v, a and t for every state of B planned paths, the forward / backward pass over squared speed under a
// speed cap, a lateral-acceleration cap, the curvature-rate limit of updateLimits, an optional clearance cap from the map stack, an optional per-state limit and
// friction-circle-coupled acceleration and braking.  The definition is the comment at po_speed_batch in include/po_hip.h; this file matches it bit for bit, so it is
// compiled with -ffp-contract=off (see Makefile) and every expression below keeps the order the definition writes.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "../../include/po_hip.h"
#include "../../include/po_pmath.h"
#define PO_MAP_DEVICE_CODE
#include "po_launch.hpp"
#include "po_map.hpp"

namespace po {

// (tests/test_speed.py places its path lengths around this: SPEED_TILE there repeats it and changes with it)
constexpr int kSpeedTile = 16;             // states per LDS tile of speed_pass_kernel
constexpr int kSpeedRow = kSpeedTile + 1;  // doubles per LDS row: odd, so the 64 lanes that walk their own rows hit 64 different bank pairs; the output sweep
                                           // uses the extra entry for state t0 + kSpeedTile (a_i reads w and s of state i + 1)

__device__ __forceinline__ double spd_min(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ double spd_max(double a, double b) { return b > a ? b : a; }
__device__ __forceinline__ bool spd_finite(double v) { return fabs(v) <= DBL_MAX; }  // false for NaN and +-inf
__device__ __forceinline__ int spd_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// One wave per path, lanes over states: W_i of step 1 into out->v (rows < n), zeros into every other entry of the v, a and t rows; the path's verdict into status
// (0: not profiled, 1: the sweeps run) and 0 into total_time.  A path that turns out non-finite has its W entries zeroed again by the lanes that wrote them.
__global__ __launch_bounds__(64) void speed_caps_kernel(DevMaps ms, DevCar c, DevSpeed a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n = spd_clamp(a.n_states ? a.n_states[b] : a.N, a.N);
    const double *st = a.states + (size_t)b * a.N * 5;
    const double *lim = a.v_limit ? a.v_limit + (size_t)b * a.N : nullptr;
    double *vrow = a.v + (size_t)b * a.N, *arow = a.a + (size_t)b * a.N, *trow = a.t ? a.t + (size_t)b * a.N : nullptr;
    const double v0 = a.v0[b];
    const bool good = (a.ok ? a.ok[b] != 0 : true) && n >= 2 && spd_finite(v0) && v0 >= 0;  // wave-uniform
    DevMap m{};
    if (a.use_map) m = map_of(ms, b);
    bool finite = true;
    for (int i = lane; i < a.N; i += 64) {
        double W = 0.0;
        if (good && i < n) {
            const double *r = st + 5 * (size_t)i;
            const double k = r[3], s = r[4];
            finite = finite && spd_finite(k) && spd_finite(s);
            W = a.v_max * a.v_max;
            const double ak = fabs(k);
            if (ak > 0) W = spd_min(W, a.a_lat_max / ak);
            double rr = 0.0;
            if (i > 0) {  // interval i - 1: rows i - 1 and i
                const double ds = s - r[-1];
                rr = spd_max(rr, ds > 0 ? fabs(k - r[-2]) / ds : 0);
            }
            if (i < n - 1) {  // interval i: rows i and i + 1
                const double ds = r[9] - s;
                rr = spd_max(rr, ds > 0 ? fabs(r[8] - k) / ds : 0);
            }
            if (rr > 0) {
                const double q = a.R / rr;
                W = spd_min(W, q * q);
            }
            if (lim) {
                const double l = lim[i];
                if (l >= 0) W = spd_min(W, l * l);
            }
            if (a.use_map) {  // c_i of po_select_batch's definition (po_select.hip): six footprint circles on the path's own layer
                const double x = r[0], y = r[1], z = r[2];
                finite = finite && spd_finite(x) && spd_finite(y) && spd_finite(z);
                const double cz = po_pcos(z), sz = po_psin(z);
                double ci = 0.0;
#pragma unroll 1
                for (int q = 0; q < 6; ++q) {
                    const double gx = (c.cx[q] * cz - c.cy[q] * sz) + x;
                    const double gy = (c.cx[q] * sz + c.cy[q] * cz) + y;
                    const double cq = map_distance(m, gx, gy) - c.cr[q];
                    ci = q == 0 ? cq : spd_min(ci, cq);
                }
                const double cc = ci > 0 ? ci : 0;
                const double vc = a.clear_v0 + a.clear_gain * cc;
                W = spd_min(W, vc * vc);
            }
        }
        vrow[i] = W;
        arow[i] = 0.0;
        if (trow) trow[i] = 0.0;
    }
    const bool valid = good && !__any(!finite);
    if (good && !valid)
        for (int i = lane; i < n; i += 64) vrow[i] = 0.0;
    if (lane == 0) {
        a.status[b] = valid ? 1 : 0;
        if (a.total_time) a.total_time[b] = 0.0;
    }
}

// One LANE per path, 64 paths per workgroup: the forward pass, the backward pass and the output sweep are dependent chains along a path, so a wave per path would
// idle 63 lanes.  Every sweep moves tiles of kSpeedTile states of its 64 paths through LDS: the wave loads them with consecutive lanes on consecutive states of one
// path (16 lanes per path, 4 paths per load), every lane then walks its own row, and the wave stores the tile the same way.  w travels through out->v between the
// sweeps.  A lane is idle beyond its own n (0 for a path speed_caps_kernel did not pass); every access is bounded by n_l[], the clamped lengths.
__global__ __launch_bounds__(64) void speed_pass_kernel(DevSpeed a) {
    __shared__ double w_l[64][kSpeedRow], k_l[64][kSpeedRow], s_l[64][kSpeedRow];
    __shared__ int n_l[64];
    constexpr int T = kSpeedTile;
    const int lane = threadIdx.x, b0 = blockIdx.x * 64, b = b0 + lane;
    int n = 0;
    if (b < a.B && a.status[b] != 0) n = spd_clamp(a.n_states ? a.n_states[b] : a.N, a.N);
    n_l[lane] = n;
    int nmax = n;
    for (int h = 32; h > 0; h >>= 1) {
        const int o = __shfl_xor(nmax, h);
        nmax = o > nmax ? o : nmax;
    }
    __syncthreads();
    if (nmax == 0) return;  // (wave-uniform)
    const double v0 = n ? a.v0[b] : 0.0;
    const double AA = a.A * a.A;

    // entries [0, cnt) of the tile at t0: w from out->v, k (when asked) and s from the rows
    auto load = [&](int t0, int cnt, bool want_k) {
        for (int idx = lane; idx < 64 * cnt; idx += 64) {
            const int p = idx / cnt, i = idx - p * cnt, gi = t0 + i;
            if (gi < n_l[p]) {
                const size_t at = (size_t)(b0 + p) * a.N + gi;
                w_l[p][i] = a.v[at];
                if (want_k) k_l[p][i] = a.states[5 * at + 3];
                s_l[p][i] = a.states[5 * at + 4];
            }
        }
        __syncthreads();
    };
    auto store_w = [&](int t0) {
        __syncthreads();
        for (int idx = lane; idx < 64 * T; idx += 64) {
            const int p = idx / T, i = idx - p * T, gi = t0 + i;
            if (gi < n_l[p]) a.v[(size_t)(b0 + p) * a.N + gi] = w_l[p][i];
        }
        __syncthreads();
    };

    // forward pass: (w, k, s) of state i - 1 ride in registers
    double wp = 0.0, kp = 0.0, sp = 0.0;
    for (int t0 = 0; t0 < nmax; t0 += T) {
        load(t0, T, true);
        for (int i = 0; i < T; ++i) {
            const int gi = t0 + i;
            if (gi < n) {
                const double W = w_l[lane][i], k = k_l[lane][i], s = s_l[lane][i];
                double w;
                if (gi == 0) {
                    w = spd_min(W, v0 * v0);
                } else {
                    const double lat = wp * fabs(kp);
                    double rem = AA - lat * lat;
                    rem = rem > 0 ? rem : 0;
                    const double ax = spd_min(sqrt(rem), a.a_max);
                    const double ds = s - sp, d = ds > 0 ? ds : 0;
                    w = spd_min(W, wp + (2 * ax) * d);
                }
                w_l[lane][i] = w;
                wp = w; kp = k; sp = s;
            }
        }
        store_w(t0);
    }

    // backward pass, tiles in reverse: (w, k, s) of state i + 1 ride in registers
    double wn = 0.0, kn = 0.0, sn = 0.0;
    for (int t0 = ((nmax - 1) / T) * T; t0 >= 0; t0 -= T) {
        load(t0, T, true);
        for (int i = T - 1; i >= 0; --i) {
            const int gi = t0 + i;
            if (gi < n) {
                double w = w_l[lane][i];
                const double k = k_l[lane][i], s = s_l[lane][i];
                if (gi == n - 1) {
                    if (a.v_end) {
                        const double e = a.v_end[b];
                        if (spd_finite(e) && e >= 0) w = spd_min(w, e * e);
                    }
                } else {
                    const double lat = wn * fabs(kn);
                    double rem = AA - lat * lat;
                    rem = rem > 0 ? rem : 0;
                    const double bx = spd_min(sqrt(rem), a.b_max);
                    const double ds = sn - s, d = ds > 0 ? ds : 0;
                    w = spd_min(w, wn + (2 * bx) * d);
                }
                w_l[lane][i] = w;
                wn = w; kn = k; sn = s;
            }
        }
        store_w(t0);
    }
    if (n) a.status[b] = wn < v0 * v0 ? 2 : 1;  // wn is the final w_0

    // outputs: v into w_l, a into k_l, t into s_l (entry i only, after its last read; entry i + 1 is still w and s), the tile stored to the three rows.  The tile
    // has kSpeedTile + 1 entries here; entry kSpeedTile is state t0 + kSpeedTile, which out->v still holds as w (only entries < kSpeedTile are stored).
    double vp = 0.0, tp = 0.0;
    sp = 0.0;
    for (int t0 = 0; t0 < nmax; t0 += T) {
        load(t0, T + 1, false);
        for (int i = 0; i < T; ++i) {
            const int gi = t0 + i;
            if (gi < n) {
                const double w = w_l[lane][i], s = s_l[lane][i];
                const double v = sqrt(w);
                double tt = 0.0, acc = 0.0;
                if (gi > 0) {
                    const double ds = s - sp, d = ds > 0 ? ds : 0;
                    const double vs = vp + v;
                    tt = tp + (vs > 0 ? (2 * d) / vs : 0);
                }
                if (gi < n - 1) {
                    const double ds = s_l[lane][i + 1] - s;
                    acc = ds > 0 ? (w_l[lane][i + 1] - w) / (2 * ds) : 0;
                    acc = spd_max(-a.A, spd_min(acc, a.A));
                }
                w_l[lane][i] = v; k_l[lane][i] = acc; s_l[lane][i] = tt;
                vp = v; tp = tt; sp = s;
            }
        }
        __syncthreads();
        for (int idx = lane; idx < 64 * T; idx += 64) {
            const int p = idx / T, i = idx - p * T, gi = t0 + i;
            if (gi < n_l[p]) {
                const size_t at = (size_t)(b0 + p) * a.N + gi;
                a.v[at] = w_l[p][i];
                a.a[at] = k_l[p][i];
                if (a.t) a.t[at] = s_l[p][i];
            }
        }
        __syncthreads();
    }
    if (n && a.total_time) a.total_time[b] = tp;
}

}  // namespace po

extern "C" hipError_t po_launch_speed(const po::DevMaps *m, const po::DevCar *c, const po::DevSpeed *a, hipStream_t st) {
    hipLaunchKernelGGL(po::speed_caps_kernel, dim3(a->B), dim3(64), 0, st, *m, *c, *a);
    hipLaunchKernelGGL(po::speed_pass_kernel, dim3((a->B + 63) / 64), dim3(64), 0, st, *a);
    return hipGetLastError();
}
