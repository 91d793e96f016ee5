// path_select.hpp — host mirror of po_select_batch (include/po_hip.h): score candidate paths on the engine's map, one winner per group.
// Header-only over the C ABI, like the other mirrors.  The reference has no such stage; the types follow its data structures (State).
#pragma once
#include <stdexcept>
#include <string>
#include <vector>

#include "data_struct.hpp"
#include "po_hip.h"
#include "solver.hpp"

namespace PathOptimizationNS {

struct SelectParams : po_select_params {
    SelectParams() { po_default_select_params(this); }  // a starting point nobody has tuned
};

struct Selection {
    std::vector<int> best;                   // [G] index into `candidates`, -1: no feasible candidate
    std::vector<double> best_cost;           // [G]
    std::vector<int> n_feasible;             // [G]
    std::vector<std::vector<State>> winners; // [G] the winners' states (empty without a winner)
    std::vector<double> cost;                // [B] +inf = infeasible
    std::vector<double> feat;                // [B][PO_N_FEAT]
};

class PathSelector {
public:
    explicit PathSelector(const SelectParams &params = SelectParams()) : params_(params) {}
    // candidates: B paths; group_sizes: G sizes that sum to at most B (group g = the next group_sizes[g] candidates); ok: empty or B flags; goals: empty or B states
    // (x, y read); previous: empty or G paths, last cycle's winners.  The engine needs a map (Map / MapStack) that covers B candidates.
    Selection select(PoEngine *engine, const std::vector<std::vector<State>> &candidates, const std::vector<int> &group_sizes, const std::vector<int> &ok = {},
                     const std::vector<State> &goals = {}, const std::vector<std::vector<State>> &previous = {}) const {
        const size_t B = candidates.size(), G = group_sizes.size();
        if ((!ok.empty() && ok.size() != B) || (!goals.empty() && goals.size() != B) || (!previous.empty() && previous.size() != G))
            throw std::invalid_argument("PathSelector::select: ok / goals need one entry per candidate, previous one per group");
        size_t N = 1, Np = 0;
        for (const auto &c : candidates) N = c.size() > N ? c.size() : N;
        for (const auto &p : previous) Np = p.size() > Np ? p.size() : Np;
        std::vector<double> st(5 * B * N, 0.0), pv(5 * G * Np, 0.0), gl(2 * goals.size());
        std::vector<int> n(B), pn(previous.size()), gs(G + 1, 0);
        pack(candidates, N, st, n);
        pack(previous, Np, pv, pn);
        for (size_t b = 0; b < goals.size(); ++b) { gl[2 * b] = goals[b].x; gl[2 * b + 1] = goals[b].y; }
        for (size_t g = 0; g < G; ++g) gs[g + 1] = gs[g] + group_sizes[g];
        Selection r;
        r.best.assign(G, -1); r.best_cost.assign(G, 0.0); r.n_feasible.assign(G, 0); r.cost.assign(B, 0.0); r.feat.assign(PO_N_FEAT * B, 0.0);
        std::vector<double> sel(5 * G * N, 0.0);
        std::vector<int> sel_n(G, 0);
        po_select_in in{};
        in.B = (int)B; in.N = (int)N; in.states = st.data(); in.n_states = n.data(); in.ok = ok.empty() ? nullptr : ok.data();
        in.goal = goals.empty() ? nullptr : gl.data(); in.goal_stride = 2; in.G = (int)G; in.group_start = gs.data();
        in.Np = (int)Np; in.prev_states = Np ? pv.data() : nullptr; in.prev_n = Np ? pn.data() : nullptr;
        po_select_out out{r.feat.data(), r.cost.data(), r.best.data(), r.best_cost.data(), r.n_feasible.data(), sel.data(), sel_n.data()};
        const int rc = po_select_batch(engine->handle(), &params_, &in, &out);
        if (rc != PO_OK) throw std::runtime_error(std::string("po_select_batch: ") + po_strerror(rc));
        r.winners.resize(G);
        for (size_t g = 0; g < G; ++g)
            for (int i = 0; i < sel_n[g]; ++i) {
                const double *row = &sel[5 * (g * N + i)];
                r.winners[g].emplace_back(row[0], row[1], row[2], row[3], row[4]);
            }
        return r;
    }

private:
    static void pack(const std::vector<std::vector<State>> &paths, size_t stride, std::vector<double> &rows, std::vector<int> &count) {
        for (size_t b = 0; b < paths.size(); ++b) {
            count[b] = (int)paths[b].size();
            for (size_t i = 0; i < paths[b].size(); ++i) {
                const State &s = paths[b][i];
                double *row = &rows[5 * (b * stride + i)];
                row[0] = s.x; row[1] = s.y; row[2] = s.z; row[3] = s.k; row[4] = s.s;
            }
        }
    }
    SelectParams params_;
};

}  // namespace PathOptimizationNS
