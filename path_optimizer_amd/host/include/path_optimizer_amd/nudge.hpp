// nudge.hpp — host mirror of po_nudge_batch (include/po_hip.h): carve predicted agents out of the corridor bounds of reference lines, pass
// LEFT or RIGHT of each, and report the agents that leave no side.  The bounds that come back go into ReferencePath::setBounds and so into
// OsqpSolver::solveBatch; the sides go into the next call's side_prev.  Header-only over the C ABI, like the other mirrors; agents are dynamic_check.hpp's.
// The reference has no such stage.
#pragma once
#include <stdexcept>
#include <string>
#include <vector>

#include "data_struct.hpp"
#include "dynamic_check.hpp"
#include "po_hip.h"
#include "solver.hpp"

namespace PathOptimizationNS {

struct NudgeParams : po_nudge_params {
    NudgeParams() { po_default_nudge_params(this); }  // a starting point nobody has tuned
};

struct Nudge {
    std::vector<int> status;                                  // [B] 0: not processed, 1: no agent touches the corridor, 2: carved, 3: at least one agent blocks
    std::vector<std::vector<CoveringCircleBounds>> bounds;    // [B] one entry per reference state: what ReferencePath::setBounds takes (x, y, heading as given)
    std::vector<std::vector<int>> side;                       // [B] per agent of the path's set: 0 untouched, +1 the vehicle passes left of it, -1 right, 2 blocks
    std::vector<int> first_blocked_state, first_blocked_agent;  // [B] -1 when none; the agent as an index over all sets in order
    std::vector<double> width_min;                            // [B] the narrowest pair of the carved corridor; DBL_MAX when not processed
    std::vector<int> ok() const {                             // [B] what PathSelector takes as ok
        std::vector<int> r(status.size());
        for (size_t b = 0; b < r.size(); ++b) r[b] = status[b] == 1 || status[b] == 2;
        return r;
    }
};

class CorridorNudger {
public:
    explicit CorridorNudger(const NudgeParams &params = NudgeParams()) : params_(params) {}
    // refs: B reference lines; t: per line, when the vehicle is expected at each state; bounds: per line, one CoveringCircleBounds per state; sets: the agent
    // sets; set_of: empty (every line meets set 0) or the set of each line; ok: empty or B flags; side_prev: empty, or per line the side vector the last call
    // returned (a row may be shorter than the set: missing entries = no hint).
    Nudge nudge(PoEngine *engine, const std::vector<std::vector<State>> &refs, const std::vector<std::vector<double>> &t,
                const std::vector<std::vector<CoveringCircleBounds>> &bounds, const std::vector<std::vector<Agent>> &sets, const std::vector<int> &set_of = {},
                const std::vector<int> &ok = {}, const std::vector<std::vector<int>> &side_prev = {}) const {
        const size_t B = refs.size();
        if (t.size() != B || bounds.size() != B || (!set_of.empty() && set_of.size() != B) || (!ok.empty() && ok.size() != B) ||
            (!side_prev.empty() && side_prev.size() != B))
            throw std::invalid_argument("CorridorNudger::nudge: t and bounds need one row per line; set_of, ok and side_prev none or one per line");
        size_t N = 1, W = 1;
        for (const auto &p : refs) N = p.size() > N ? p.size() : N;
        for (const auto &s : sets) W = s.size() > W ? s.size() : W;
        std::vector<double> rx(B * N, 0.0), ry(B * N, 0.0), rz(B * N, 0.0), tt(B * N, 0.0), bin(8 * B * N, 0.0), bout(8 * B * N, 0.0);
        std::vector<int> n(B), prev(side_prev.empty() ? 0 : B * W, 0);
        for (size_t b = 0; b < B; ++b) {
            if (t[b].size() != refs[b].size() || bounds[b].size() != refs[b].size())
                throw std::invalid_argument("CorridorNudger::nudge: a line needs one time and one CoveringCircleBounds per state");
            n[b] = (int)refs[b].size();
            for (size_t i = 0; i < refs[b].size(); ++i) {
                const size_t o = b * N + i;
                rx[o] = refs[b][i].x; ry[o] = refs[b][i].y; rz[o] = refs[b][i].z; tt[o] = t[b][i];
                const CoveringCircleBounds::SingleCircleBounds *c[4] = {&bounds[b][i].c0, &bounds[b][i].c1, &bounds[b][i].c2, &bounds[b][i].c3};
                for (int j = 0; j < 4; ++j) { bin[o * 8 + 2 * j] = c[j]->lb; bin[o * 8 + 2 * j + 1] = c[j]->ub; }
            }
            if (!side_prev.empty())
                for (size_t e = 0; e < side_prev[b].size() && e < W; ++e) prev[b * W + e] = side_prev[b][e];
        }
        std::vector<po_agent> flat;
        std::vector<int> first;
        pack_agent_sets(sets, "CorridorNudger::nudge", &flat, &first);
        Nudge r;
        r.status.assign(B, 0); r.first_blocked_state.assign(B, -1); r.first_blocked_agent.assign(B, -1); r.width_min.assign(B, 0.0);
        r.bounds = bounds; r.side.resize(B);
        if (B == 0) return r;
        std::vector<int> side(B * W, 0);
        po_agent_lists lists{flat.empty() ? nullptr : flat.data(), first.data(), (int)flat.size(), (int)sets.size()};
        po_nudge_in in{};
        in.B = (int)B; in.N = (int)N; in.W = (int)W; in.ref_x = rx.data(); in.ref_y = ry.data(); in.ref_z = rz.data(); in.n_points = n.data();
        in.ok = ok.empty() ? nullptr : ok.data(); in.t = tt.data(); in.bounds = bin.data(); in.set_of = set_of.empty() ? nullptr : set_of.data();
        in.agents = &lists; in.side_prev = side_prev.empty() ? nullptr : prev.data();
        po_nudge_out out{};
        out.status = r.status.data(); out.bounds = bout.data(); out.side = side.data(); out.first_blocked_state = r.first_blocked_state.data();
        out.first_blocked_agent = r.first_blocked_agent.data(); out.width_min = r.width_min.data();
        const int rc = po_nudge_batch(engine->handle(), &params_, &in, &out);
        if (rc != PO_OK) throw std::runtime_error(std::string("po_nudge_batch: ") + po_strerror(rc));
        for (size_t b = 0; b < B; ++b) {
            for (size_t i = 0; i < refs[b].size(); ++i) {
                const size_t o = b * N + i;
                CoveringCircleBounds::SingleCircleBounds *c[4] = {&r.bounds[b][i].c0, &r.bounds[b][i].c1, &r.bounds[b][i].c2, &r.bounds[b][i].c3};
                for (int j = 0; j < 4; ++j) { c[j]->lb = bout[o * 8 + 2 * j]; c[j]->ub = bout[o * 8 + 2 * j + 1]; }
            }
            const int k = set_of.empty() ? 0 : set_of[b];
            const size_t cnt = (k >= 0 && (size_t)k < sets.size()) ? sets[k].size() : 0;
            r.side[b].assign(side.begin() + b * W, side.begin() + b * W + cnt);
        }
        return r;
    }

private:
    NudgeParams params_;
};

}  // namespace PathOptimizationNS
