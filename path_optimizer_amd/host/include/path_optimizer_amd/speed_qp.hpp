// speed_qp.hpp — host mirror of po_speedqp_batch (include/po_hip.h): a jerk-limited s(t) inside the tunnel a station-time plan leaves free.
// Takes the paths, the plan (stations per layer, as StGoPlan::station holds them), the planner's samples and, when there is one, its cell map, and returns the
// smoothed samples as States (x, y, z, k, s, v, a) with jerk, times and the tunnel — what DynamicChecker::check and TrajectorySampler::sample read.
// Header-only over the C ABI, like the other mirrors.  The reference has no such stage.
#pragma once
#include <stdexcept>
#include <string>
#include <vector>

#include "data_struct.hpp"
#include "po_hip.h"
#include "solver.hpp"

namespace PathOptimizationNS {

struct SpeedQpParams : po_speedqp_params {
    SpeedQpParams() { po_default_speedqp_params(this); }  // a starting point nobody has tuned
};

struct SpeedQpResult {
    std::vector<int> status;                  // [B] 0: not run, 1: converged, 2: max_iter reached (the iterate is written)
    std::vector<int> iters, n_fact, n_q;      // [B]
    std::vector<double> r_prim, r_dual;       // [B] the residuals of the last check
    std::vector<std::vector<State>> samples;  // [B][Q] x, y, z, k, s, v, a of every sample (all zero when not run)
    std::vector<std::vector<double>> jerk, t, lo, hi;  // [B][Q]; lo and hi relative to the path's first s
    std::vector<std::vector<int>> index;      // [B][Q] the state a sample is anchored at, -1 when not run
};

class SpeedQp {
public:
    explicit SpeedQp(const SpeedQpParams &params = SpeedQpParams()) : params_(params) {}
    // paths: B paths (s non-decreasing); v0: B speeds; station: B plans, station[b] = the n_layers + 1 stations of the plan (empty: no plan, the path is not run);
    // ref_s: B rows of Q reference arc lengths (the planner's samples' s); cells: empty or B * K * PO_ST_MAX_STATIONS entries; v_cap: empty or B rows.
    SpeedQpResult solve(PoEngine *engine, const std::vector<std::vector<State>> &paths, const std::vector<double> &v0, const std::vector<std::vector<int>> &station,
                        const std::vector<std::vector<double>> &ref_s, const std::vector<int> &cells = {}, const std::vector<std::vector<double>> &v_cap = {}) const {
        const size_t B = paths.size(), Q = params_.Q > 0 ? (size_t)params_.Q : 0, K = params_.K > 0 ? (size_t)params_.K : 0, W = PO_ST_MAX_LAYERS + 1;
        if (v0.size() != B || station.size() != B || ref_s.size() != B || (!v_cap.empty() && v_cap.size() != B) ||
            (!cells.empty() && cells.size() != B * K * PO_ST_MAX_STATIONS))
            throw std::invalid_argument("SpeedQp::solve: v0, station and ref_s need one entry per path; cells and v_cap none or one per path");
        size_t N = 1;
        for (const auto &p : paths) N = p.size() > N ? p.size() : N;
        std::vector<double> st(5 * B * N, 0.0), cap(v_cap.empty() ? 0 : B * N, -1.0), ref(5 * B * Q, 0.0);
        std::vector<int> n(B), ok(B, 1), stn(B * W, -1), nl(B, 0);
        for (size_t b = 0; b < B; ++b) {
            n[b] = (int)paths[b].size();
            for (size_t i = 0; i < paths[b].size(); ++i) {
                const State &s = paths[b][i];
                double *row = &st[5 * (b * N + i)];
                row[0] = s.x; row[1] = s.y; row[2] = s.z; row[3] = s.k; row[4] = s.s;
            }
            if (!v_cap.empty())
                for (size_t i = 0; i < v_cap[b].size() && i < N; ++i) cap[b * N + i] = v_cap[b][i];
            if (station[b].size() > W || ref_s[b].size() != Q) throw std::invalid_argument("SpeedQp::solve: a plan has at most 17 stations, a reference row Q entries");
            if (station[b].size() < 2) ok[b] = 0;
            else nl[b] = (int)station[b].size() - 1;
            for (size_t k = 0; k < station[b].size(); ++k) stn[b * W + k] = station[b][k];
            for (size_t q = 0; q < Q; ++q) ref[5 * (b * Q + q) + 4] = ref_s[b][q];
        }
        SpeedQpResult r;
        r.status.assign(B, 0); r.iters.assign(B, 0); r.n_fact.assign(B, 0); r.n_q.assign(B, 0); r.r_prim.assign(B, 0.0); r.r_dual.assign(B, 0.0);
        r.samples.resize(B); r.jerk.resize(B); r.t.resize(B); r.lo.resize(B); r.hi.resize(B); r.index.resize(B);
        if (B == 0) return r;
        std::vector<double> os(5 * B * Q), ov(B * Q), oa(B * Q), oj(B * Q), ot(B * Q), lo(B * Q), hi(B * Q);
        std::vector<int> oi(B * Q);
        po_speedqp_in in{};
        in.B = (int)B; in.N = (int)N; in.states = st.data(); in.n_states = n.data(); in.ok = ok.data(); in.v0 = v0.data(); in.v_cap = v_cap.empty() ? nullptr : cap.data();
        in.station = stn.data(); in.n_layers = nl.data(); in.cells = cells.empty() ? nullptr : cells.data(); in.ref_states = ref.data();
        po_speedqp_out out{};
        out.status = r.status.data(); out.iters = r.iters.data(); out.n_fact = r.n_fact.data(); out.r_prim = r.r_prim.data(); out.r_dual = r.r_dual.data();
        out.n_q = r.n_q.data(); out.states = os.data(); out.v = ov.data(); out.a = oa.data(); out.jerk = oj.data(); out.t = ot.data(); out.lo = lo.data();
        out.hi = hi.data(); out.index = oi.data();
        const int rc = po_speedqp_batch(engine->handle(), &params_, &in, &out);
        if (rc != PO_OK) throw std::runtime_error(std::string("po_speedqp_batch: ") + po_strerror(rc));
        for (size_t b = 0; b < B; ++b) {
            r.samples[b].reserve(Q);
            for (size_t q = 0; q < Q; ++q) {
                const double *row = &os[5 * (b * Q + q)];
                r.samples[b].emplace_back(row[0], row[1], row[2], row[3], row[4], ov[b * Q + q], oa[b * Q + q]);
            }
            r.jerk[b].assign(oj.begin() + b * Q, oj.begin() + (b + 1) * Q);
            r.t[b].assign(ot.begin() + b * Q, ot.begin() + (b + 1) * Q);
            r.lo[b].assign(lo.begin() + b * Q, lo.begin() + (b + 1) * Q);
            r.hi[b].assign(hi.begin() + b * Q, hi.begin() + (b + 1) * Q);
            r.index[b].assign(oi.begin() + b * Q, oi.begin() + (b + 1) * Q);
        }
        return r;
    }

private:
    SpeedQpParams params_;
};

}  // namespace PathOptimizationNS
