// st_go.hpp — host mirror of po_stgo_batch (include/po_hip.h): station-time plans that may resume after a stop — drive, stop, wait, go —
// handed over sampled at uniform time steps as States (x, y, z, k, s, v, a), which DynamicChecker::check and TrajectorySampler::sample read with the sample
// times.  Header-only over the C ABI, like the other mirrors; agents are dynamic_check.hpp's.  The reference has no such stage.
#pragma once
#include <stdexcept>
#include <string>
#include <vector>

#include "data_struct.hpp"
#include "dynamic_check.hpp"
#include "po_hip.h"
#include "solver.hpp"

namespace PathOptimizationNS {

struct StGoParams : po_stgo_params {
    StGoParams() { po_default_stgo_params(this); }  // a starting point nobody has tuned
};

struct StGoPlan {
    std::vector<int> status;                  // [B] 0: not planned, 1: planned and no cell blocked, 2: planned around blocked cells, 3: no plan
    std::vector<int> n_layers;                // [B] steps of the chosen plan
    std::vector<double> cost;                 // [B] DBL_MAX without a plan
    std::vector<std::vector<int>> station;    // [B] the station at every step of the plan (n_layers + 1 entries; empty without a plan)
    std::vector<int> n_resumes;               // [B] times the plan pulls away after a window at rest
    std::vector<std::vector<State>> samples;  // [B][Q] x, y, z, k, s, v, a of every sample (all zero without a plan)
    std::vector<std::vector<double>> t;       // [B][Q] the sample times (zero without a plan)
    std::vector<std::vector<int>> index;      // [B][Q] the state a sample is anchored at, -1 without a plan
    std::vector<int> first_held;              // [B] the first sample behind the plan's last layer; Q when none; -1 without a plan
    std::vector<int> end;                     // [B] 0: no plan, 1: the samples end inside the plan, 2: held arrived, 3: held at rest, 4: held at speed
    std::vector<int> ok() const {             // [B] what PathSelector takes as ok
        std::vector<int> r(status.size());
        for (size_t b = 0; b < r.size(); ++b) r[b] = status[b] == 1 || status[b] == 2;
        return r;
    }
};

class StGoPlanner {
public:
    explicit StGoPlanner(const StGoParams &params = StGoParams()) : params_(params) {}
    // paths: B paths (s non-decreasing); v0: the B speeds the vehicles have now; sets: the agent sets; set_of: empty (every path meets set 0) or the set of each
    // path; ok: empty or B flags; v_cap: empty or B rows of per-state speed caps.  A row of v_cap may be shorter than its path; missing entries = none.
    StGoPlan plan(PoEngine *engine, const std::vector<std::vector<State>> &paths, const std::vector<double> &v0, const std::vector<std::vector<Agent>> &sets,
                  const std::vector<int> &set_of = {}, const std::vector<int> &ok = {}, const std::vector<std::vector<double>> &v_cap = {}) const {
        const size_t B = paths.size();
        if (v0.size() != B || (!set_of.empty() && set_of.size() != B) || (!ok.empty() && ok.size() != B) || (!v_cap.empty() && v_cap.size() != B))
            throw std::invalid_argument("StGoPlanner::plan: v0 needs one entry per path; set_of, ok and v_cap none or one per path");
        size_t N = 1;
        for (const auto &p : paths) N = p.size() > N ? p.size() : N;
        std::vector<double> st(5 * B * N, 0.0), cap(v_cap.empty() ? 0 : B * N, -1.0);
        std::vector<int> n(B);
        for (size_t b = 0; b < B; ++b) {
            n[b] = (int)paths[b].size();
            for (size_t i = 0; i < paths[b].size(); ++i) {
                const State &s = paths[b][i];
                double *row = &st[5 * (b * N + i)];
                row[0] = s.x; row[1] = s.y; row[2] = s.z; row[3] = s.k; row[4] = s.s;
            }
            if (!v_cap.empty())
                for (size_t i = 0; i < v_cap[b].size() && i < N; ++i) cap[b * N + i] = v_cap[b][i];
        }
        std::vector<po_agent> flat;
        std::vector<int> first;
        pack_agent_sets(sets, "StGoPlanner::plan", &flat, &first);
        StGoPlan r;
        r.status.assign(B, 0); r.n_layers.assign(B, 0); r.cost.assign(B, 0.0); r.station.resize(B); r.n_resumes.assign(B, 0);
        r.samples.resize(B); r.t.resize(B); r.index.resize(B); r.first_held.assign(B, 0); r.end.assign(B, 0);
        if (B == 0) return r;
        const size_t Q = params_.Q > 0 ? (size_t)params_.Q : 0;
        std::vector<int> station(B * (PO_ST_MAX_LAYERS + 1)), oi(B * Q);
        std::vector<double> os(5 * B * Q), ov(B * Q), oa(B * Q), ot(B * Q);
        po_agent_lists lists{flat.empty() ? nullptr : flat.data(), first.data(), (int)flat.size(), (int)sets.size()};
        po_stgo_in in{};
        in.B = (int)B; in.N = (int)N; in.states = st.data(); in.n_states = n.data(); in.ok = ok.empty() ? nullptr : ok.data(); in.v0 = v0.data();
        in.v_cap = v_cap.empty() ? nullptr : cap.data(); in.set_of = set_of.empty() ? nullptr : set_of.data(); in.agents = &lists;
        po_stgo_out out{};
        out.status = r.status.data(); out.n_layers = r.n_layers.data(); out.cost = r.cost.data(); out.station = station.data(); out.n_resumes = r.n_resumes.data();
        out.states = os.data(); out.v = ov.data(); out.a = oa.data(); out.t = ot.data(); out.index = oi.data(); out.first_held = r.first_held.data();
        out.end = r.end.data();
        const int rc = po_stgo_batch(engine->handle(), &params_, &in, &out);
        if (rc != PO_OK) throw std::runtime_error(std::string("po_stgo_batch: ") + po_strerror(rc));
        for (size_t b = 0; b < B; ++b) {
            const int *s = &station[b * (PO_ST_MAX_LAYERS + 1)];
            if (r.status[b] == 1 || r.status[b] == 2) r.station[b].assign(s, s + r.n_layers[b] + 1);
            r.samples[b].reserve(Q);
            for (size_t q = 0; q < Q; ++q) {
                const double *row = &os[5 * (b * Q + q)];
                r.samples[b].emplace_back(row[0], row[1], row[2], row[3], row[4], ov[b * Q + q], oa[b * Q + q]);
            }
            r.t[b].assign(ot.begin() + b * Q, ot.begin() + (b + 1) * Q);
            r.index[b].assign(oi.begin() + b * Q, oi.begin() + (b + 1) * Q);
        }
        return r;
    }

private:
    StGoParams params_;
};

}  // namespace PathOptimizationNS
