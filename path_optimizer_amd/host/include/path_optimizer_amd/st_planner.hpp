// st_planner.hpp — host mirror of po_stplan_batch (include/po_hip.h): station-time speed planning of paths against agents on predicted
// trajectories — pass ahead, ease off or stop — and the v_limit rows that hand the plan to SpeedProfiler::profile.  Header-only over the C ABI, like the other
// mirrors; agents are dynamic_check.hpp's.  The reference has no such stage.
#pragma once
#include <stdexcept>
#include <string>
#include <vector>

#include "data_struct.hpp"
#include "dynamic_check.hpp"
#include "po_hip.h"
#include "solver.hpp"

namespace PathOptimizationNS {

struct StPlanParams : po_stplan_params {
    StPlanParams() { po_default_stplan_params(this); }  // a starting point nobody has tuned
};

struct StPlan {
    std::vector<int> status;                   // [B] 0: not planned, 1: planned and no cell blocked, 2: planned around blocked cells, 3: no plan
    std::vector<int> n_layers;                 // [B] steps of the chosen plan
    std::vector<double> cost;                  // [B] DBL_MAX without a plan
    std::vector<std::vector<int>> station;     // [B] the station at every step of the plan (n_layers + 1 entries; empty without a plan)
    std::vector<std::vector<int>> cells;       // [B] K rows of PO_ST_MAX_STATIONS: the agent that blocks (window, station), -1: free
    std::vector<std::vector<double>> v_limit;  // [B] per state: what SpeedProfiler::profile takes as v_limit
    std::vector<int> ok() const {              // [B] what PathSelector takes as ok
        std::vector<int> r(status.size());
        for (size_t b = 0; b < r.size(); ++b) r[b] = status[b] == 1 || status[b] == 2;
        return r;
    }
};

class StPlanner {
public:
    explicit StPlanner(const StPlanParams &params = StPlanParams()) : params_(params) {}
    // paths: B paths; v0: the B speeds the vehicles have now; sets: the agent sets; set_of: empty (every path meets set 0) or the set of each path; ok: empty or
    // B flags; v_cap: empty or B rows of per-state speed caps (SpeedProfile's v of a profile without agents); v_limit_in: empty or B rows merged into the result's
    // v_limit.  A row of v_cap or v_limit_in may be shorter than its path; missing entries = none.
    StPlan plan(PoEngine *engine, const std::vector<std::vector<State>> &paths, const std::vector<double> &v0, const std::vector<std::vector<Agent>> &sets,
                const std::vector<int> &set_of = {}, const std::vector<int> &ok = {}, const std::vector<std::vector<double>> &v_cap = {},
                const std::vector<std::vector<double>> &v_limit_in = {}) const {
        const size_t B = paths.size();
        if (v0.size() != B || (!set_of.empty() && set_of.size() != B) || (!ok.empty() && ok.size() != B) || (!v_cap.empty() && v_cap.size() != B) ||
            (!v_limit_in.empty() && v_limit_in.size() != B))
            throw std::invalid_argument("StPlanner::plan: v0 needs one entry per path; set_of, ok, v_cap and v_limit_in none or one per path");
        size_t N = 1;
        for (const auto &p : paths) N = p.size() > N ? p.size() : N;
        std::vector<double> st(5 * B * N, 0.0), cap(v_cap.empty() ? 0 : B * N, -1.0), lim(v_limit_in.empty() ? 0 : B * N, -1.0);
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
            if (!v_limit_in.empty())
                for (size_t i = 0; i < v_limit_in[b].size() && i < N; ++i) lim[b * N + i] = v_limit_in[b][i];
        }
        std::vector<po_agent> flat;
        std::vector<int> first;
        pack_agent_sets(sets, "StPlanner::plan", &flat, &first);
        StPlan r;
        r.status.assign(B, 0); r.n_layers.assign(B, 0); r.cost.assign(B, 0.0); r.station.resize(B); r.cells.resize(B); r.v_limit.resize(B);
        if (B == 0) return r;
        const size_t K = params_.K > 0 ? (size_t)params_.K : 0, row = K * PO_ST_MAX_STATIONS;
        std::vector<int> station(B * (PO_ST_MAX_LAYERS + 1)), cells(B * row);
        std::vector<double> vl(B * N);
        po_agent_lists lists{flat.empty() ? nullptr : flat.data(), first.data(), (int)flat.size(), (int)sets.size()};
        po_stplan_in in{};
        in.B = (int)B; in.N = (int)N; in.states = st.data(); in.n_states = n.data(); in.ok = ok.empty() ? nullptr : ok.data(); in.v0 = v0.data();
        in.v_cap = v_cap.empty() ? nullptr : cap.data(); in.set_of = set_of.empty() ? nullptr : set_of.data(); in.agents = &lists;
        in.v_limit_in = v_limit_in.empty() ? nullptr : lim.data();
        po_stplan_out out{};
        out.status = r.status.data(); out.n_layers = r.n_layers.data(); out.cost = r.cost.data(); out.station = station.data(); out.cells = cells.data();
        out.v_limit = vl.data();
        const int rc = po_stplan_batch(engine->handle(), &params_, &in, &out);
        if (rc != PO_OK) throw std::runtime_error(std::string("po_stplan_batch: ") + po_strerror(rc));
        for (size_t b = 0; b < B; ++b) {
            const int *s = &station[b * (PO_ST_MAX_LAYERS + 1)];
            if (r.status[b] == 1 || r.status[b] == 2) r.station[b].assign(s, s + r.n_layers[b] + 1);
            r.cells[b].assign(cells.begin() + b * row, cells.begin() + (b + 1) * row);
            r.v_limit[b].assign(vl.begin() + b * N, vl.begin() + b * N + paths[b].size());
        }
        return r;
    }

private:
    StPlanParams params_;
};

}  // namespace PathOptimizationNS
