// dynamic_check.hpp — host mirror of po_dynamic_batch (include/po_hip.h): timed paths against agents on predicted trajectories, the first
// conflict of every path and the v_limit rows that make SpeedProfiler::profile stop short of it.  Header-only over the C ABI, like the other mirrors.  The
// reference has no such stage.
#pragma once
#include <stdexcept>
#include <string>
#include <vector>

#include "data_struct.hpp"
#include "po_hip.h"
#include "solver.hpp"

namespace PathOptimizationNS {

struct DynamicParams : po_dynamic_params {
    DynamicParams() { po_default_dynamic_params(this); }  // a starting point nobody has tuned
};

// A disc of `radius` that moves along (t, x, y) points, linear in time between them; 1 .. PO_AGENT_MAX_PTS points, t strictly increasing.
struct Agent {
    double radius = 0.0;
    bool hold_before = false, hold_after = false;  // present at the first point before its time / at the last point after its time
    std::vector<double> t, x, y;
    Agent() = default;
    Agent(double r, bool before, bool after) : radius(r), hold_before(before), hold_after(after) {}
    void add(double ti, double xi, double yi) { t.push_back(ti); x.push_back(xi); y.push_back(yi); }  // (one point with both flags: a static disc)
};

// sets -> the arrays of po_agent_lists: set k owns flat[first[k] .. first[k + 1]).  `who` names the caller ("Class::method") in the exception.
inline void pack_agent_sets(const std::vector<std::vector<Agent>> &sets, const char *who, std::vector<po_agent> *flat, std::vector<int> *first) {
    flat->clear();
    first->assign(1, 0);
    for (const auto &set : sets) {
        for (const Agent &a : set) {
            if (a.t.empty() || a.t.size() > PO_AGENT_MAX_PTS || a.x.size() != a.t.size() || a.y.size() != a.t.size())
                throw std::invalid_argument(std::string(who) + ": an agent has 1 .. 8 points (t, x, y)");
            po_agent g{};
            g.n_pts = (int)a.t.size();
            g.flags = (a.hold_before ? PO_AGENT_HOLD_BEFORE : 0) | (a.hold_after ? PO_AGENT_HOLD_AFTER : 0);
            g.radius = a.radius;
            for (size_t j = 0; j < a.t.size(); ++j) { g.t[j] = a.t[j]; g.x[j] = a.x[j]; g.y[j] = a.y[j]; }
            flat->push_back(g);
        }
        first->push_back((int)flat->size());
    }
}

struct DynamicResult {
    std::vector<int> status;                    // [B] 0: not checked, 1: free, 2: conflict, 3: conflict nearer than stop_distance
    std::vector<int> first_state, first_agent;  // [B] the first conflicting interval and its agent (index into the concatenated sets), -1 when free
    std::vector<int> stop_state;                // [B]
    std::vector<double> first_time, gap_min;    // [B]
    std::vector<std::vector<double>> gap;       // [B] per interval (one entry per state; DBL_MAX where nothing was evaluated)
    std::vector<std::vector<double>> v_limit;   // [B] per state: what SpeedProfiler::profile takes as v_limit
    std::vector<int> ok() const {               // [B] what PathSelector takes as ok
        std::vector<int> r(status.size());
        for (size_t b = 0; b < r.size(); ++b) r[b] = status[b] == 1;
        return r;
    }
};

class DynamicChecker {
public:
    explicit DynamicChecker(const DynamicParams &params = DynamicParams()) : params_(params) {}
    // paths: B paths; t: the B time rows SpeedProfiler::profile returned (SpeedProfile::t); sets: the agent sets; set_of: empty (every path meets set 0) or the set
    // of each path; ok: empty or B flags; v_limit_in: empty or B rows merged into the result's v_limit (a row may be shorter than its path; missing entries = none).
    DynamicResult check(PoEngine *engine, const std::vector<std::vector<State>> &paths, const std::vector<std::vector<double>> &t,
                        const std::vector<std::vector<Agent>> &sets, const std::vector<int> &set_of = {}, const std::vector<int> &ok = {},
                        const std::vector<std::vector<double>> &v_limit_in = {}) const {
        const size_t B = paths.size();
        if (t.size() != B || (!set_of.empty() && set_of.size() != B) || (!ok.empty() && ok.size() != B) || (!v_limit_in.empty() && v_limit_in.size() != B))
            throw std::invalid_argument("DynamicChecker::check: t needs one row per path; set_of, ok and v_limit_in none or one per path");
        size_t N = 1;
        for (const auto &p : paths) N = p.size() > N ? p.size() : N;
        std::vector<double> st(5 * B * N, 0.0), tt(B * N, 0.0), lim(v_limit_in.empty() ? 0 : B * N, -1.0);
        std::vector<int> n(B);
        for (size_t b = 0; b < B; ++b) {
            if (t[b].size() != paths[b].size()) throw std::invalid_argument("DynamicChecker::check: a time row needs one entry per state");
            n[b] = (int)paths[b].size();
            for (size_t i = 0; i < paths[b].size(); ++i) {
                const State &s = paths[b][i];
                double *row = &st[5 * (b * N + i)];
                row[0] = s.x; row[1] = s.y; row[2] = s.z; row[3] = s.k; row[4] = s.s;
                tt[b * N + i] = t[b][i];
            }
            if (!v_limit_in.empty())
                for (size_t i = 0; i < v_limit_in[b].size() && i < N; ++i) lim[b * N + i] = v_limit_in[b][i];
        }
        std::vector<po_agent> flat;
        std::vector<int> first;
        pack_agent_sets(sets, "DynamicChecker::check", &flat, &first);
        DynamicResult r;
        r.status.assign(B, 0); r.first_state.assign(B, -1); r.first_agent.assign(B, -1); r.stop_state.assign(B, -1);
        r.first_time.assign(B, 0.0); r.gap_min.assign(B, 0.0); r.gap.resize(B); r.v_limit.resize(B);
        if (B == 0) return r;
        std::vector<double> gap(B * N), vl(B * N);
        po_agent_lists lists{flat.empty() ? nullptr : flat.data(), first.data(), (int)flat.size(), (int)sets.size()};
        po_dynamic_in in{};
        in.B = (int)B; in.N = (int)N; in.states = st.data(); in.n_states = n.data(); in.ok = ok.empty() ? nullptr : ok.data(); in.t = tt.data();
        in.set_of = set_of.empty() ? nullptr : set_of.data(); in.agents = &lists; in.v_limit_in = v_limit_in.empty() ? nullptr : lim.data();
        po_dynamic_out out{};
        out.status = r.status.data(); out.gap_min = r.gap_min.data(); out.first_state = r.first_state.data(); out.first_agent = r.first_agent.data();
        out.stop_state = r.stop_state.data(); out.first_time = r.first_time.data(); out.gap = gap.data(); out.v_limit = vl.data();
        const int rc = po_dynamic_batch(engine->handle(), &params_, &in, &out);
        if (rc != PO_OK) throw std::runtime_error(std::string("po_dynamic_batch: ") + po_strerror(rc));
        for (size_t b = 0; b < B; ++b) {
            r.gap[b].assign(gap.begin() + b * N, gap.begin() + b * N + paths[b].size());
            r.v_limit[b].assign(vl.begin() + b * N, vl.begin() + b * N + paths[b].size());
        }
        return r;
    }

private:
    DynamicParams params_;
};

}  // namespace PathOptimizationNS
