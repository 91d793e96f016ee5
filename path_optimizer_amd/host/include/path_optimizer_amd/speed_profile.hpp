// speed_profile.hpp — host mirror of po_speed_batch (include/po_hip.h): a speed, an acceleration and a time for every state of planned paths.
// Header-only over the C ABI, like the other mirrors.  The reference has no such stage; it only consumes State.v / State.a (ReferencePathImpl::updateLimits), which
// this fills.
#pragma once
#include <stdexcept>
#include <string>
#include <vector>

#include "data_struct.hpp"
#include "po_hip.h"
#include "solver.hpp"

namespace PathOptimizationNS {

struct SpeedParams : po_speed_params {
    SpeedParams() { po_default_speed_params(this); }  // a starting point nobody has tuned
};

struct SpeedProfile {
    std::vector<std::vector<double>> t;  // [B] time at every state of the path (all zero for a path that was not profiled)
    std::vector<double> total_time;      // [B]
    std::vector<int> status;             // [B] 0: not profiled, 1: profiled, 2: profiled, and the vehicle enters faster than the profile allows
};

class SpeedProfiler {
public:
    explicit SpeedProfiler(const SpeedParams &params = SpeedParams()) : params_(params) {}
    // paths: B paths, State.v / State.a are FILLED; v0: B start speeds; v_end: empty or B end speeds (a negative entry = free); ok: empty or B flags; v_limit: empty or
    // B rows of per-state limits (a row may be shorter than its path; missing and negative entries = none).  With params.use_map the engine needs a map (Map /
    // MapStack) that covers B paths; without it no map is read.
    SpeedProfile profile(PoEngine *engine, std::vector<std::vector<State>> &paths, const std::vector<double> &v0, const std::vector<double> &v_end = {},
                         const std::vector<int> &ok = {}, const std::vector<std::vector<double>> &v_limit = {}) const {
        const size_t B = paths.size();
        if (v0.size() != B || (!v_end.empty() && v_end.size() != B) || (!ok.empty() && ok.size() != B) || (!v_limit.empty() && v_limit.size() != B))
            throw std::invalid_argument("SpeedProfiler::profile: v0 needs one entry per path; v_end, ok and v_limit none or one per path");
        size_t N = 1;
        for (const auto &p : paths) N = p.size() > N ? p.size() : N;
        std::vector<double> st(5 * B * N, 0.0), lim(v_limit.empty() ? 0 : B * N, -1.0), v(B * N), a(B * N), t(B * N);
        std::vector<int> n(B);
        for (size_t b = 0; b < B; ++b) {
            n[b] = (int)paths[b].size();
            for (size_t i = 0; i < paths[b].size(); ++i) {
                const State &s = paths[b][i];
                double *row = &st[5 * (b * N + i)];
                row[0] = s.x; row[1] = s.y; row[2] = s.z; row[3] = s.k; row[4] = s.s;
            }
            if (!v_limit.empty())
                for (size_t i = 0; i < v_limit[b].size() && i < N; ++i) lim[b * N + i] = v_limit[b][i];
        }
        SpeedProfile r;
        r.total_time.assign(B, 0.0); r.status.assign(B, 0); r.t.resize(B);
        if (B == 0) return r;
        po_speed_in in{};
        in.B = (int)B; in.N = (int)N; in.states = st.data(); in.n_states = n.data(); in.ok = ok.empty() ? nullptr : ok.data();
        in.v0 = v0.data(); in.v_end = v_end.empty() ? nullptr : v_end.data(); in.v_limit = v_limit.empty() ? nullptr : lim.data();
        po_speed_out out{v.data(), a.data(), t.data(), r.total_time.data(), r.status.data()};
        const int rc = po_speed_batch(engine->handle(), &params_, &in, &out);
        if (rc != PO_OK) throw std::runtime_error(std::string("po_speed_batch: ") + po_strerror(rc));
        for (size_t b = 0; b < B; ++b) {
            r.t[b].assign(t.begin() + b * N, t.begin() + b * N + paths[b].size());
            for (size_t i = 0; i < paths[b].size(); ++i) { paths[b][i].v = v[b * N + i]; paths[b][i].a = a[b * N + i]; }
        }
        return r;
    }

private:
    SpeedParams params_;
};

}  // namespace PathOptimizationNS
