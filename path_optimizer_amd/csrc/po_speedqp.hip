// po_speedqp.hip — speed QP: the tunnel lo_q <= s(T_q) - S_0 <= hi_q a station-time plan leaves free, and a piecewise-jerk QP inside it solved
// by OSQP's ADMM, unscaled, with a banded LDL^T of half-bandwidth 3.  The definition is the comment at po_speedqp_batch in include/po_hip.h; this file matches it
// bit for bit, so it is compiled with -ffp-contract=off (see Makefile) and every expression below keeps the order the definition writes.
//
// One wave per path.  Everything of a path lives in LDS sized from Q (kSqpArrays rows of Q doubles): the row operations — A x, A^T w, the projections, the norms —
// are lanes over samples or rows, each evaluating the nested differences of the definition from the LDS rows around its index; the three chains (factorisation,
// forward and backward substitution) run on lane 0 with the running values in registers, their last product the only dependent one.  No atomics, no scratch.
#include <hip/hip_runtime.h>

#include "po_launch.hpp"
#include "po_map.hpp"

namespace po {

constexpr int kSqpThreads = 64;
constexpr int kSqpArrays = 31;  // x, xt, qv; z, y, l, u, rr and w by row class (4 each); K0 / D, K1 / L1, K2 / L2, K3 / L3
static_assert((size_t)kSqpArrays * PO_SQP_MAX_SAMPLES * sizeof(double) <= kLdsLimit, "speedqp_kernel's LDS at the limit of Q");

__device__ __forceinline__ unsigned long long sqp_abs_bits(double v) { return (unsigned long long)__double_as_longlong(v) & 0x7fffffffffffffffull; }

// The largest of the lanes' bit patterns, in every lane (all 64 lanes call it)
__device__ __forceinline__ unsigned long long sqp_wave_max(unsigned long long v) {
    for (int h = 32; h > 0; h >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)(v & 0xffffffffull), h), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), h);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o > v ? o : v;
    }
    return v;
}

// ---- A: the rows of a vector given by an accessor x(r) ----
template <class X> __device__ __forceinline__ double sqp_e(const X &x, int r) {
    const double d = x(r + 1) - x(r), dm = r > 0 ? x(r) - x(r - 1) : 0.0;
    return d - dm;
}
template <class X> __device__ __forceinline__ double sqp_row_v(const X &x, int r, double i1) { return (x(r + 1) - x(r)) * i1; }
template <class X> __device__ __forceinline__ double sqp_row_a(const X &x, int r, double i2) { return sqp_e(x, r) * i2; }
template <class X> __device__ __forceinline__ double sqp_row_j(const X &x, int r, double i3) { return (sqp_e(x, r + 1) - sqp_e(x, r)) * i3; }

// ---- A^T: entry q for row values given by accessors (called only on rows that exist) ----
template <class WP, class WV, class WA, class WJ>
__device__ __forceinline__ double sqp_cols(int q, int n, const WP &wp, const WV &wv, const WA &wa, const WJ &wj, double i1, double i2, double i3) {
    auto pj = [&](int r) { return (r >= 1 && r <= n - 3) ? wj(r) * i3 : 0.0; };
    auto ta = [&](int r) { return (r >= 0 && r <= n - 2) ? wa(r) * i2 + (pj(r - 1) - pj(r)) : 0.0; };
    auto tv = [&](int r) { return (r >= 0 && r <= n - 2) ? wv(r) * i1 + (ta(r) - ta(r + 1)) : 0.0; };
    return wp(q) + (tv(q - 1) - tv(q));
}

struct SqpRows {  // the LDS rows of one path
    double *x, *xt, *qv, *z[4], *y[4], *l[4], *u[4], *rr[4], *w[4], *kb[4];
};

// rr: rho per row (1e3 * rho on equality rows).  Lanes over rows; the caller synchronises.
__device__ __forceinline__ void sqp_row_rho(const SqpRows &R, int n, double rho) {
    const int lane = threadIdx.x;
    for (int c = 0; c < 4; ++c) {
        const int r0 = c == 3 ? 1 : 0, r1 = c == 0 ? n - 1 : (c == 3 ? n - 3 : n - 2);
        for (int r = r0 + lane; r <= r1; r += kSqpThreads)
            R.rr[c][r] = __double_as_longlong(R.l[c][r]) == __double_as_longlong(R.u[c][r]) ? 1e3 * rho : rho;
    }
}

// The band of K from the operators on unit vectors (lanes over columns), then the factorisation in place on lane 0.  Starts and ends with a barrier.
__device__ __forceinline__ void sqp_factor(const SqpRows &R, int n, double gsig, double twa, double twj, double i1, double i2, double i3) {
    const int lane = threadIdx.x;
    __syncthreads();
    for (int c = lane; c < n; c += kSqpThreads) {
        auto x = [&](int r) { return r == c ? 1.0 : 0.0; };
        auto wp = [&](int r) { return (R.rr[0][r] + gsig) * x(r); };
        auto wv = [&](int r) { return R.rr[1][r] * sqp_row_v(x, r, i1); };
        auto wa = [&](int r) { return (R.rr[2][r] + twa) * sqp_row_a(x, r, i2); };
        auto wj = [&](int r) { return (R.rr[3][r] + twj) * sqp_row_j(x, r, i3); };
        for (int k = 0; k < 4; ++k) R.kb[k][c] = c + k < n ? sqp_cols(c + k, n, wp, wv, wa, wj, i1, i2, i3) : 0.0;
    }
    __syncthreads();
    if (lane == 0) {
        double *D = R.kb[0], *L1 = R.kb[1], *L2 = R.kb[2], *L3 = R.kb[3];
        // (Lk * D) of the three columns behind j: a = column j - 1, b = j - 2, c = j - 3
        double l1a = 0, l2a = 0, l3a = 0, da = 0, l2b = 0, l3b = 0, db = 0, l3c = 0, dc = 0;
        for (int j = 0; j < n; ++j) {
            double d = D[j], c1 = L1[j], c2 = L2[j];
            if (j >= 1) d = d - (l1a * da) * l1a;
            if (j >= 2) d = d - (l2b * db) * l2b;
            if (j >= 3) d = d - (l3c * dc) * l3c;
            if (j >= 1) c1 = c1 - (l2a * da) * l1a;
            if (j >= 2) c1 = c1 - (l3b * db) * l2b;
            if (j >= 1) c2 = c2 - (l3a * da) * l1a;
            const double n1 = c1 / d, n2 = c2 / d, n3 = L3[j] / d;
            D[j] = d; L1[j] = n1; L2[j] = n2; L3[j] = n3;
            l3c = l3b; dc = db;
            l2b = l2a; l3b = l3a; db = da;
            l1a = n1; l2a = n2; l3a = n3; da = d;
        }
    }
    __syncthreads();
}

// Not run: zeros, index -1
__device__ __forceinline__ void sqp_not_run(const DevSpeedQp &a, int b) {
    const int lane = threadIdx.x, Q = a.Q;
    for (int q = lane; q < Q; q += kSqpThreads) {
        const size_t o = (size_t)b * Q + q;
        double *w = a.o_states + 5 * o;
        w[0] = 0.0; w[1] = 0.0; w[2] = 0.0; w[3] = 0.0; w[4] = 0.0;
        if (a.o_v) a.o_v[o] = 0.0;
        if (a.o_a) a.o_a[o] = 0.0;
        if (a.o_jerk) a.o_jerk[o] = 0.0;
        if (a.o_t) a.o_t[o] = 0.0;
        if (a.o_lo) a.o_lo[o] = 0.0;
        if (a.o_hi) a.o_hi[o] = 0.0;
        if (a.index) a.index[o] = -1;
    }
    if (lane == 0) {
        a.status[b] = 0;
        if (a.iters) a.iters[b] = 0;
        if (a.n_fact) a.n_fact[b] = 0;
        if (a.r_prim) a.r_prim[b] = 0.0;
        if (a.r_dual) a.r_dual[b] = 0.0;
        if (a.n_q) a.n_q[b] = 0;
    }
}

// Every barrier is reached by the whole wave: the early returns and the loop exits are uniform.
__global__ __launch_bounds__(kSqpThreads) void speedqp_kernel(DevSpeedQp a) {
    extern __shared__ double sqp_lds[];
    __shared__ int stn[PO_ST_MAX_LAYERS + 1];
    const int lane = threadIdx.x, b = blockIdx.x, Q = a.Q, N = a.N, stride = a.stride;
    const double *st = a.states + (size_t)b * N * 5;

    // ---- what is run ----
    int n = a.n_states ? a.n_states[b] : N;
    n = n < 0 ? 0 : (n > N ? N : n);
    const double v0 = a.v0[b];
    bool run = !(a.ok && a.ok[b] == 0) && n >= 2 && (v0 >= 0 && v0 - v0 == 0);
    int bad = 0;
    if (run)
        for (int i = lane; i < n; i += kSqpThreads) {
            const double *r = st + 5 * (size_t)i;
            const double fin = ((r[0] - r[0]) + (r[1] - r[1])) + ((r[2] - r[2]) + (r[4] - r[4]));  // 0 exactly when all four are finite (a predicate, not a value)
            if (!(fin == 0)) bad = 1;
            if (i + 1 < n && r[9] < r[4]) bad = 1;
        }
    bad = __syncthreads_or(bad);
    int M = n >= 1 ? (n - 1) / stride + 1 : 0;
    M = M > PO_ST_MAX_STATIONS ? PO_ST_MAX_STATIONS : M;
    int nl = a.n_layers[b];
    nl = nl < 0 ? 0 : (nl > a.K ? a.K : nl);
    run = run && !bad && M >= 2 && nl >= 1;
    if (run) {  // (uniform)
        if (lane <= nl) {
            const int s = a.station[(size_t)b * (PO_ST_MAX_LAYERS + 1) + lane];
            stn[lane] = s < 0 ? 0 : (s > PO_ST_MAX_STATIONS - 1 ? PO_ST_MAX_STATIONS - 1 : s);
        }
        __syncthreads();
        for (int k = 0; k < nl; ++k) run = run && !(stn[k + 1] < stn[k]);
        run = run && !(stn[nl] > M - 1);
    }
    const double dt = a.dt, h = a.dts;
    int nq = 0;
    if (run) {
        const double Tend = (double)nl * dt;
        for (int q = lane; q < Q; q += kSqpThreads) nq += ((double)q * h <= Tend) ? 1 : 0;
        for (int s = 32; s > 0; s >>= 1) nq += __shfl_xor(nq, s);
        const double *ref = a.ref_states + (size_t)b * Q * 5;
        int nf = 0;
        for (int q = lane; q < nq; q += kSqpThreads) {
            const double r = ref[5 * (size_t)q + 4];
            if (!(r - r == 0)) nf = 1;
        }
        run = !__syncthreads_or(nf);
    }
    if (!run) {  // (uniform)
        sqp_not_run(a, b);
        return;
    }

    SqpRows R;
    {
        double *p = sqp_lds;
        R.x = p; p += Q; R.xt = p; p += Q; R.qv = p; p += Q;
        for (int c = 0; c < 4; ++c) { R.z[c] = p; p += Q; R.y[c] = p; p += Q; R.l[c] = p; p += Q; R.u[c] = p; p += Q; R.rr[c] = p; p += Q; R.w[c] = p; p += Q; R.kb[c] = p; p += Q; }
    }
    const int nn = nq;
    const double S0 = st[4];
    const double i1 = 1.0 / h, i2 = i1 / h, i3 = i2 / h;
    const double tws = 2.0 * a.w_s, twa = 2.0 * a.w_a, twj = 2.0 * a.w_j;
    const double c0 = v0 * i1;
    auto S = [&](int m) { return st[5 * (size_t)(m * stride) + 4]; };
    auto Vc = [&](int m) {
        double v = a.v_max;
        if (a.v_cap) {
            const double e = a.v_cap[(size_t)b * N + (size_t)m * stride];
            if (e >= 0) v = e < v ? e : v;
        }
        return v;
    };

    // ---- the tunnel, the bounds, qv; x = z = y = 0 ----
    for (int q = lane; q < nn; q += kSqpThreads) {
        const double T = (double)q * h;
        int kk = 0;
        for (int k = 1; k <= nl; ++k)
            if ((double)k * dt <= T) kk = k;
        double lo = 0.0, hi = 0.0;
        bool first = true;
        for (int t = 0; t < 2; ++t) {
            const int w = t == 0 ? kk - 1 : kk;
            if (t == 0 && !(kk >= 1 && T == (double)kk * dt)) continue;
            if (w > nl - 1) continue;
            const int p = stn[w], j = stn[w + 1];
            int lo_m = 0, hi_m = M - 1;
            if (a.cells) {
                const int *row = a.cells + ((size_t)b * a.K + w) * PO_ST_MAX_STATIONS;
                for (int m = p - 1; m >= 0; --m)
                    if (row[m] >= 0) { lo_m = m + 1; break; }
                for (int m = j + 1; m < M; ++m)
                    if (row[m] >= 0) { hi_m = m - 1; break; }
            }
            const double al = S(lo_m) - S0, ah = S(hi_m) - S0;
            if (first) { lo = al; hi = ah; first = false; }
            else { lo = al > lo ? al : lo; hi = ah < hi ? ah : hi; }
        }
        if (q == 0) { lo = 0.0; hi = 0.0; }
        R.l[0][q] = lo; R.u[0][q] = hi;
        if (q < nn - 1) {
            const int w = kk < nl - 1 ? kk : nl - 1;
            double c = Vc(stn[w]);
            for (int m = stn[w] + 1; m <= stn[w + 1]; ++m) {
                const double e = Vc(m);
                c = e < c ? e : c;
            }
            R.l[1][q] = 0.0; R.u[1][q] = c;
            R.l[2][q] = q == 0 ? -a.b_max + c0 : -a.b_max;
            R.u[2][q] = q == 0 ? a.a_max + c0 : a.a_max;
        }
        if (q >= 1 && q <= nn - 3) { R.l[3][q] = -a.j_max; R.u[3][q] = a.j_max; }
        R.x[q] = 0.0;
        for (int c = 0; c < 4; ++c) { R.z[c][q] = 0.0; R.y[c][q] = 0.0; }
    }
    int status = 1, it = 0, n_fact = 0;
    double rp = 0.0, rd = 0.0, rho = a.rho;
    if (nn >= 2) {  // (uniform)
        const double *ref = a.ref_states + (size_t)b * Q * 5;
        auto zero = [](int) { return 0.0; };
        auto cv = [&](int r) { return r == 0 ? twa * c0 : 0.0; };
        unsigned long long nqb = 0;
        for (int q = lane; q < nn; q += kSqpThreads) {
            const double rq = ref[5 * (size_t)q + 4] - S0;
            const double lin = tws * rq + sqp_cols(q, nn, zero, zero, cv, zero, i1, i2, i3);
            R.qv[q] = -lin;
            const unsigned long long ab = sqp_abs_bits(-lin);
            nqb = ab > nqb ? ab : nqb;
        }
        const double nqv = __longlong_as_double((long long)sqp_wave_max(nqb));
        __syncthreads();
        sqp_row_rho(R, nn, rho);
        sqp_factor(R, nn, tws + a.sigma, twa, twj, i1, i2, i3);
        n_fact = 1;
        const double sigma = a.sigma, alpha = a.alpha, om = 1.0 - a.alpha;
        const double *D = R.kb[0], *L1 = R.kb[1], *L2 = R.kb[2], *L3 = R.kb[3];
        auto xs = [&](int r) { return R.x[r]; };
        auto xts = [&](int r) { return R.xt[r]; };
        status = 2;
        for (it = 1; it <= a.max_iter; ++it) {
            // w = rho_r * z_r - y_r by row, then rhs into xt
            for (int c = 0; c < 4; ++c) {
                const int r0 = c == 3 ? 1 : 0, r1 = c == 0 ? nn - 1 : (c == 3 ? nn - 3 : nn - 2);
                for (int r = r0 + lane; r <= r1; r += kSqpThreads) R.w[c][r] = R.rr[c][r] * R.z[c][r] - R.y[c][r];
            }
            __syncthreads();
            for (int q = lane; q < nn; q += kSqpThreads)
                R.xt[q] = (sigma * R.x[q] - R.qv[q]) + sqp_cols(q, nn, [&](int r) { return R.w[0][r]; }, [&](int r) { return R.w[1][r]; }, [&](int r) { return R.w[2][r]; },
                                                               [&](int r) { return R.w[3][r]; }, i1, i2, i3);
            __syncthreads();
            if (lane == 0) {  // forward: the three values behind q in registers
                double y1 = 0, y2 = 0, y3 = 0;
                for (int q = 0; q < nn; ++q) {
                    double t = R.xt[q];
                    if (q >= 3) t = t - L3[q - 3] * y3;
                    if (q >= 2) t = t - L2[q - 2] * y2;
                    if (q >= 1) t = t - L1[q - 1] * y1;
                    R.xt[q] = t;
                    y3 = y2; y2 = y1; y1 = t;
                }
            }
            __syncthreads();
            for (int q = lane; q < nn; q += kSqpThreads) R.xt[q] = R.xt[q] / D[q];
            __syncthreads();
            if (lane == 0) {  // backward
                double x1 = 0, x2 = 0, x3 = 0;
                for (int q = nn - 1; q >= 0; --q) {
                    double t = R.xt[q];
                    if (q + 3 < nn) t = t - L3[q] * x3;
                    if (q + 2 < nn) t = t - L2[q] * x2;
                    if (q + 1 < nn) t = t - L1[q] * x1;
                    R.xt[q] = t;
                    x3 = x2; x2 = x1; x1 = t;
                }
            }
            __syncthreads();
            for (int q = lane; q < nn; q += kSqpThreads) R.x[q] = alpha * R.xt[q] + om * R.x[q];
            for (int c = 0; c < 4; ++c) {
                const int r0 = c == 3 ? 1 : 0, r1 = c == 0 ? nn - 1 : (c == 3 ? nn - 3 : nn - 2);
                for (int r = r0 + lane; r <= r1; r += kSqpThreads) {
                    const double zt = c == 0 ? R.xt[r] : (c == 1 ? sqp_row_v(xts, r, i1) : (c == 2 ? sqp_row_a(xts, r, i2) : sqp_row_j(xts, r, i3)));
                    const double rr = R.rr[c][r], yo = R.y[c][r], l = R.l[c][r], u = R.u[c][r];
                    const double zr = alpha * zt + om * R.z[c][r];
                    const double zc = zr + yo / rr;
                    double zn = l > zc ? l : zc;
                    zn = u < zn ? u : zn;
                    R.y[c][r] = yo + rr * (zr - zn);
                    R.z[c][r] = zn;
                }
            }
            __syncthreads();
            if (it % a.check_every != 0 && it != a.max_iter) continue;  // (uniform)

            // ---- the check: w = the cost rows of P x, then the norms ----
            unsigned long long b_rp = 0, b_ax = 0, b_z = 0, b_rd = 0, b_px = 0, b_aty = 0;
            auto up = [](unsigned long long &m, double v) { const unsigned long long ab = sqp_abs_bits(v); m = ab > m ? ab : m; };
            for (int c = 0; c < 4; ++c) {
                const int r0 = c == 3 ? 1 : 0, r1 = c == 0 ? nn - 1 : (c == 3 ? nn - 3 : nn - 2);
                for (int r = r0 + lane; r <= r1; r += kSqpThreads) {
                    const double ax = c == 0 ? R.x[r] : (c == 1 ? sqp_row_v(xs, r, i1) : (c == 2 ? sqp_row_a(xs, r, i2) : sqp_row_j(xs, r, i3)));
                    up(b_rp, ax - R.z[c][r]); up(b_ax, ax); up(b_z, R.z[c][r]);
                    if (c == 2) R.w[2][r] = twa * ax;
                    if (c == 3) R.w[3][r] = twj * ax;
                }
            }
            __syncthreads();
            for (int q = lane; q < nn; q += kSqpThreads) {
                const double px = tws * R.x[q] + sqp_cols(q, nn, zero, zero, [&](int r) { return R.w[2][r]; }, [&](int r) { return R.w[3][r]; }, i1, i2, i3);
                const double aty = sqp_cols(q, nn, [&](int r) { return R.y[0][r]; }, [&](int r) { return R.y[1][r]; }, [&](int r) { return R.y[2][r]; },
                                            [&](int r) { return R.y[3][r]; }, i1, i2, i3);
                up(b_rd, (px + R.qv[q]) + aty); up(b_px, px); up(b_aty, aty);
            }
            rp = __longlong_as_double((long long)sqp_wave_max(b_rp));
            rd = __longlong_as_double((long long)sqp_wave_max(b_rd));
            const double nax = __longlong_as_double((long long)sqp_wave_max(b_ax)), nz = __longlong_as_double((long long)sqp_wave_max(b_z));
            const double npx = __longlong_as_double((long long)sqp_wave_max(b_px)), naty = __longlong_as_double((long long)sqp_wave_max(b_aty));
            const double mp = nz > nax ? nz : nax;
            double md = naty > npx ? naty : npx;
            md = nqv > md ? nqv : md;
            const double ep = a.eps_abs + a.eps_rel * mp, ed = a.eps_abs + a.eps_rel * md;
            __syncthreads();  // (w is written again at the top of the loop)
            if (rp <= ep && rd <= ed) { status = 1; break; }  // (uniform: every lane holds the same norms)
            if (it == a.max_iter) break;
            if (a.adaptive_rho) {
                double rn = rho * sqrt((rp / mp) / (rd / md));
                rn = 1e-6 > rn ? 1e-6 : rn;
                rn = 1e6 < rn ? 1e6 : rn;
                if (rn > 5.0 * rho || rn < rho / 5.0) {
                    rho = rn;
                    sqp_row_rho(R, nn, rho);
                    sqp_factor(R, nn, tws + a.sigma, twa, twj, i1, i2, i3);
                    ++n_fact;
                }
            }
        }
        if (it > a.max_iter) it = a.max_iter;
    } else {
        __syncthreads();
    }

    // ---- the samples from the iterate ----
    const double s0 = st[4], sN = st[5 * (size_t)(n - 1) + 4];
    for (int q = lane; q < Q; q += kSqpThreads) {
        const int qq = q < nn ? q : nn - 1;
        auto vel = [&](int r) { return r == 0 ? v0 : (R.x[r] - R.x[r - 1]) / h; };
        auto acc = [&](int r) { return r < nn - 1 ? (vel(r + 1) - vel(r)) / h : 0.0; };
        const double sq = S0 + R.x[qq];
        double sx = sq < s0 ? s0 : sq;
        sx = sx > sN ? sN : sx;
        int lo = 0, hi = n - 1;
        while (hi - lo > 1) {
            const int mid = lo + ((hi - lo) >> 1);
            if (st[5 * (size_t)mid + 4] <= sx) lo = mid; else hi = mid;
        }
        const double *r = st + 5 * (size_t)lo;
        const double ds = r[9] - r[4];
        double lam = ds > 0 ? (sx - r[4]) / ds : 0;
        lam = lam < 0 ? 0 : lam;
        lam = lam > 1 ? 1 : lam;
        const size_t o = (size_t)b * Q + q;
        double *w = a.o_states + 5 * o;
        w[0] = r[0] + lam * (r[5] - r[0]);
        w[1] = r[1] + lam * (r[6] - r[1]);
        w[3] = r[3] + lam * (r[8] - r[3]);
        w[4] = r[4] + lam * ds;
        double dz = r[7] - r[2];
        if (dz > 3.141592653589793) dz = dz - 6.283185307179586;
        else if (dz < -3.141592653589793) dz = dz + 6.283185307179586;
        w[2] = r[2] + lam * dz;
        if (a.o_v) a.o_v[o] = vel(qq);
        if (a.o_a) a.o_a[o] = q < nn ? acc(q) : 0.0;
        if (a.o_jerk) a.o_jerk[o] = q < nn - 2 ? (acc(q + 1) - acc(q)) / h : 0.0;
        if (a.o_t) a.o_t[o] = (double)q * h;
        if (a.o_lo) a.o_lo[o] = R.l[0][qq];
        if (a.o_hi) a.o_hi[o] = R.u[0][qq];
        if (a.index) a.index[o] = lo;
    }
    if (lane == 0) {
        a.status[b] = status;
        if (a.iters) a.iters[b] = it;
        if (a.n_fact) a.n_fact[b] = n_fact;
        if (a.r_prim) a.r_prim[b] = rp;
        if (a.r_dual) a.r_dual[b] = rd;
        if (a.n_q) a.n_q[b] = nn;
    }
}

}  // namespace po

extern "C" hipError_t po_launch_speedqp(const po::DevSpeedQp *a, hipStream_t st) {
    const size_t lds = (size_t)po::kSqpArrays * a->Q * sizeof(double);
    if (a->Q < 2 || a->Q > PO_SQP_MAX_SAMPLES || lds > po::kLdsLimit) return hipErrorInvalidValue;  // (the entry's ranges keep it inside)
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&po::speedqp_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(po::speedqp_kernel, dim3(a->B), dim3(po::kSqpThreads), lds, st, *a);
    return hipGetLastError();
}
