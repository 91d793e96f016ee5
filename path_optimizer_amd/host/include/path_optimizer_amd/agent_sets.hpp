// agent_sets.hpp — host mirror of po_agentsets_batch (include/po_hip.h): for every ego path the agents that can matter to it — the records
// of its pool (world) of the fleet's own plans (TrajectorySampler's agents) that are not its own, and of a perception list, that come near the path in space and
// in time — as the sets DynamicChecker, StPlanner and CorridorNudger take.  Header-only over the C ABI, like the other mirrors.  The reference has no such stage.
#pragma once
#include <stdexcept>
#include <string>
#include <vector>

#include "data_struct.hpp"
#include "dynamic_check.hpp"
#include "po_hip.h"
#include "solver.hpp"

namespace PathOptimizationNS {

struct AgentSetsParams : po_agentsets_params {
    AgentSetsParams() { po_default_agentsets_params(this); }  // a starting point nobody has tuned
};

struct ComposedSets {
    std::vector<int> status;      // [B] 0: not composed (an empty set), 1: complete (compose() sizes the buffer from a counting call, so never 2)
    std::vector<int> count;       // [B] records kept for each ego
    std::vector<int> first;       // [B + 1] ego b owns records [first[b], first[b + 1])
    std::vector<int> set_of;      // [B] b: what the consumers take as set_of
    std::vector<int> src_index;   // [total] where a record came from: its index among the fleet's records, or their number plus its index among perception's
    std::vector<po_agent> records;  // [total] the records as the stage copied them
    long long total = 0;
    std::vector<std::vector<Agent>> sets() const {  // [B] the sets as DynamicChecker::check, StPlanner::plan and CorridorNudger::nudge take them (set_of: this->set_of)
        std::vector<std::vector<Agent>> out(count.size());
        for (size_t b = 0; b < count.size(); ++b)
            for (int p = first[b]; p < first[b + 1]; ++p) {
                const po_agent &g = records[p];
                Agent a(g.radius, (g.flags & PO_AGENT_HOLD_BEFORE) != 0, (g.flags & PO_AGENT_HOLD_AFTER) != 0);
                for (int j = 0; j < g.n_pts; ++j) a.add(g.t[j], g.x[j], g.y[j]);
                out[b].push_back(a);
            }
        return out;
    }
};

class AgentSets {
public:
    explicit AgentSets(const AgentSetsParams &params = AgentSetsParams()) : params_(params) {}
    // paths: B ego paths; t: the B time rows SpeedProfiler::profile returned, or empty (the window of the parameters); fleet: the fleet's agents in pools (record a of
    // the concatenated pools belongs to ego a / owner_div, or to owner[a] when owner is given); perception: empty, or agents nobody owns, in pools; pool_of: empty
    // (every ego draws from pool 0) or the pool of each ego; ok: empty or B flags.
    ComposedSets compose(PoEngine *engine, const std::vector<std::vector<State>> &paths, const std::vector<std::vector<double>> &t,
                         const std::vector<std::vector<Agent>> &fleet, const std::vector<std::vector<Agent>> &perception = {}, const std::vector<int> &pool_of = {},
                         const std::vector<int> &owner = {}, const std::vector<int> &ok = {}) const {
        const size_t B = paths.size();
        if ((!t.empty() && t.size() != B) || (!pool_of.empty() && pool_of.size() != B) || (!ok.empty() && ok.size() != B))
            throw std::invalid_argument("AgentSets::compose: t, pool_of and ok none or one per path");
        size_t N = 1;
        for (const auto &p : paths) N = p.size() > N ? p.size() : N;
        std::vector<double> st(5 * B * N, 0.0), tt(t.empty() ? 0 : B * N, 0.0);
        std::vector<int> n(B);
        for (size_t b = 0; b < B; ++b) {
            if (!t.empty() && t[b].size() != paths[b].size()) throw std::invalid_argument("AgentSets::compose: a time row needs one entry per state");
            n[b] = (int)paths[b].size();
            for (size_t i = 0; i < paths[b].size(); ++i) {
                const State &s = paths[b][i];
                double *row = &st[5 * (b * N + i)];
                row[0] = s.x; row[1] = s.y; row[2] = s.z; row[3] = s.k; row[4] = s.s;
                if (!t.empty()) tt[b * N + i] = t[b][i];
            }
        }
        std::vector<po_agent> flat0, flat1;
        std::vector<int> first0, first1;
        pack_agent_sets(fleet, "AgentSets::compose", &flat0, &first0);
        pack_agent_sets(perception, "AgentSets::compose", &flat1, &first1);
        if (!owner.empty() && owner.size() != flat0.size()) throw std::invalid_argument("AgentSets::compose: owner none or one per fleet record");
        ComposedSets r;
        r.status.assign(B, 0); r.count.assign(B, 0); r.first.assign(B + 1, 0); r.set_of.assign(B, 0);
        if (B == 0) return r;
        const po_agent_lists l0{flat0.empty() ? nullptr : flat0.data(), first0.data(), (int)flat0.size(), (int)fleet.size()};
        const po_agent_lists l1{flat1.empty() ? nullptr : flat1.data(), first1.data(), (int)flat1.size(), (int)perception.size()};
        po_agentsets_in in{};
        in.B = (int)B; in.N = (int)N; in.states = st.data(); in.n_states = n.data(); in.ok = ok.empty() ? nullptr : ok.data(); in.t = t.empty() ? nullptr : tt.data();
        in.src[0] = &l0; in.src[1] = perception.empty() ? nullptr : &l1;
        in.pool_of = pool_of.empty() ? nullptr : pool_of.data(); in.owner = owner.empty() ? nullptr : owner.data();
        po_agentsets_out out{};
        out.first = r.first.data(); out.count = r.count.data(); out.status = r.status.data(); out.set_of = r.set_of.data(); out.total = &r.total;
        int rc = po_agentsets_batch(engine->handle(), &params_, &in, &out);  // capacity 0: the counting call
        if (rc == PO_OK && r.total > 0) {
            if (r.total > 0x7fffffffLL) throw std::runtime_error("AgentSets::compose: the sets do not fit one call");
            r.records.resize((size_t)r.total); r.src_index.resize((size_t)r.total);
            out.capacity = (int)r.total; out.agents = r.records.data(); out.src_index = r.src_index.data();
            rc = po_agentsets_batch(engine->handle(), &params_, &in, &out);
        }
        if (rc != PO_OK) throw std::runtime_error(std::string("po_agentsets_batch: ") + po_strerror(rc));
        return r;
    }
    // The device flavour: every array inside in, in.src[] and out is a device pointer; enqueued on the engine's stream, no synchronisation.  out.agents, out.first
    // and out.set_of are what po_dynamic_batch_device, po_stplan_batch_device and po_nudge_batch_device take.
    void composeDevice(PoEngine *engine, const po_agentsets_in &in, const po_agentsets_out &out) const {
        const int rc = po_agentsets_batch_device(engine->handle(), &params_, &in, &out);
        if (rc != PO_OK) throw std::runtime_error(std::string("po_agentsets_batch_device: ") + po_strerror(rc));
    }

private:
    AgentSetsParams params_;
};

}  // namespace PathOptimizationNS
