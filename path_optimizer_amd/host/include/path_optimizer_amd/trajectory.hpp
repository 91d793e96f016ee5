// trajectory.hpp — host mirror of po_trajectory_batch (include/po_hip.h): speed-profiled paths sampled at uniform time steps, and the same
// samples as Agents (dynamic_check.hpp's) that DynamicChecker, StPlanner and CorridorNudger take as a set: one vehicle's plan is another vehicle's agents.
// Header-only over the C ABI, like the other mirrors.  The reference has no such stage.
#pragma once
#include <stdexcept>
#include <string>
#include <vector>

#include "data_struct.hpp"
#include "dynamic_check.hpp"
#include "po_hip.h"
#include "solver.hpp"

namespace PathOptimizationNS {

struct TrajectoryParams : po_trajectory_params {
    TrajectoryParams() { po_default_trajectory_params(this); }  // a starting point nobody has tuned
};

struct Trajectory {
    std::vector<int> status;                  // [B] 0: not sampled, 1: the horizon lies inside the path's time span, 2: held at rest, 3: held at speed (the path ends first)
    std::vector<int> first_held;              // [B] the first sample that is held; K when none; -1 when not sampled
    std::vector<std::vector<State>> samples;  // [B][K] x, y, z, k, s, v, a of every sample (all zero for a path that was not sampled)
    std::vector<std::vector<double>> t;       // [B][K] the sample times
    std::vector<std::vector<int>> index;      // [B][K] the state a sample is anchored at, -1 when not sampled
    std::vector<std::vector<Agent>> agents;   // [B] the n_discs agents of each path: a set per vehicle (empty for a path that was not sampled and with n_discs = 0)
};

class TrajectorySampler {
public:
    explicit TrajectorySampler(const TrajectoryParams &params = TrajectoryParams()) : params_(params) {}
    // paths: B paths with State.v as SpeedProfiler::profile filled it; t: the B time rows it returned (SpeedProfile::t); ok: empty or B flags.
    Trajectory sample(PoEngine *engine, const std::vector<std::vector<State>> &paths, const std::vector<std::vector<double>> &t, const std::vector<int> &ok = {}) const {
        const size_t B = paths.size();
        if (t.size() != B || (!ok.empty() && ok.size() != B)) throw std::invalid_argument("TrajectorySampler::sample: t needs one row per path; ok none or one per path");
        size_t N = 1;
        for (const auto &p : paths) N = p.size() > N ? p.size() : N;
        const size_t K = params_.K > 0 ? (size_t)params_.K : 0, D = params_.n_discs > 0 ? (size_t)params_.n_discs : 0;
        std::vector<double> st(5 * B * N, 0.0), v(B * N, 0.0), tt(B * N, 0.0);
        std::vector<int> n(B);
        for (size_t b = 0; b < B; ++b) {
            if (t[b].size() != paths[b].size()) throw std::invalid_argument("TrajectorySampler::sample: a time row needs one entry per state");
            n[b] = (int)paths[b].size();
            for (size_t i = 0; i < paths[b].size(); ++i) {
                const State &s = paths[b][i];
                double *row = &st[5 * (b * N + i)];
                row[0] = s.x; row[1] = s.y; row[2] = s.z; row[3] = s.k; row[4] = s.s;
                v[b * N + i] = s.v; tt[b * N + i] = t[b][i];
            }
        }
        Trajectory r;
        r.status.assign(B, 0); r.first_held.assign(B, -1);
        r.samples.resize(B); r.t.resize(B); r.index.resize(B); r.agents.resize(B);
        if (B == 0) return r;
        std::vector<double> os(5 * B * K), ov(B * K), oa(B * K), ot(B * K);
        std::vector<int> oi(B * K);
        std::vector<po_agent> rec(B * D);
        po_trajectory_in in{};
        in.B = (int)B; in.N = (int)N; in.states = st.data(); in.n_states = n.data(); in.ok = ok.empty() ? nullptr : ok.data(); in.v = v.data(); in.t = tt.data();
        po_trajectory_out out{};
        out.status = r.status.data(); out.states = os.data(); out.v = ov.data(); out.a = oa.data(); out.t = ot.data(); out.index = oi.data();
        out.first_held = r.first_held.data(); out.agents = D ? rec.data() : nullptr;
        const int rc = po_trajectory_batch(engine->handle(), &params_, &in, &out);
        if (rc != PO_OK) throw std::runtime_error(std::string("po_trajectory_batch: ") + po_strerror(rc));
        for (size_t b = 0; b < B; ++b) {
            r.t[b].assign(ot.begin() + b * K, ot.begin() + (b + 1) * K);
            r.index[b].assign(oi.begin() + b * K, oi.begin() + (b + 1) * K);
            for (size_t k = 0; k < K; ++k) {
                const double *row = &os[5 * (b * K + k)];
                State s(row[0], row[1], row[2], row[3], row[4]);
                s.v = ov[b * K + k]; s.a = oa[b * K + k];
                r.samples[b].push_back(s);
            }
            for (size_t d = 0; d < D && r.status[b] != 0; ++d) {
                const po_agent &g = rec[b * D + d];
                Agent a(g.radius, (g.flags & PO_AGENT_HOLD_BEFORE) != 0, (g.flags & PO_AGENT_HOLD_AFTER) != 0);
                for (int j = 0; j < g.n_pts; ++j) a.add(g.t[j], g.x[j], g.y[j]);
                r.agents[b].push_back(a);
            }
        }
        return r;
    }

private:
    TrajectoryParams params_;
};

}  // namespace PathOptimizationNS
