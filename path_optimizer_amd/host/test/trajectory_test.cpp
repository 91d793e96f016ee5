// The timed trajectory through the host mirror (trajectory.hpp): TrajectorySampler::sample on a small seeded case — 6 profiled paths of 1 .. 27 states 0.5 m
// apart at 1 .. 3 m/s with the clock of po_speed_batch, one of them stopped for good from state 5 on, one with ok = 0; 40 samples every 0.125 s from -0.25 s,
// two discs per path as agents of four points, the stride at its limit.  Every number comes from an integer generator and dyadic arithmetic (the clock's one
// division is the same operation in both languages), so tests/test_trajectory.py rebuilds the same case bit for bit and compares the statuses, first_held and
// the checksums printed here with Engine.trajectory_batch and the reference.  No map is set: the stage reads none.  Checked here: the shapes, that a path
// with ok = 0 comes back empty, that s never decreases along the samples, that held samples sit on a state of the path, and that the agents can be handed to
// DynamicChecker as sets.  Exit code 0 = passed.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "path_optimizer_amd/trajectory.hpp"

using namespace PathOptimizationNS;

namespace {
unsigned lcg_state = 24680u;
double u() {  // a multiple of 1 / 64 in [-2, 2]
    lcg_state = (lcg_state * 1103515245u + 12345u) & 0x7fffffffu;
    return ((int)((lcg_state >> 8) % 257u) - 128) / 64.0;
}
bool expect(bool ok, const char *what) {
    if (!ok) std::printf("FAILED: %s\n", what);
    return ok;
}
uint64_t bits(double v) {
    uint64_t b;
    std::memcpy(&b, &v, sizeof b);
    return b;
}
}  // namespace

int main() {
    const int B = 6;
    PoEngine engine(0);
    std::vector<std::vector<State>> paths(B);
    std::vector<std::vector<double>> t(B);
    for (int b = 0; b < B; ++b) {
        double tt = u() / 4;
        for (int i = 0; i < 1 + (b * 11) % 29; ++i) {
            const double x = -6.0 + 0.5 * i + u() / 16;
            const double y = u() / 2;
            const double z = u() / 8;
            const double k = u() / 32;
            double vv = 2.0 + u() / 2;
            if (b == 2 && i >= 5) vv = 0.0;
            if (i > 0) {
                const double vs = paths[b][i - 1].v + vv;
                tt = tt + (vs > 0 ? 1.0 / vs : 0.0);
            }
            paths[b].emplace_back(x, y, z, k, 0.5 * i, vv);
            t[b].push_back(tt);
        }
    }
    std::vector<int> ok(B, 1);
    ok[4] = 0;

    TrajectoryParams tp;
    tp.t0 = -0.25; tp.dt = 0.125; tp.K = 40; tp.n_discs = 2; tp.disc_offset[0] = -0.5; tp.disc_offset[1] = 1.5; tp.disc_radius[0] = 1.25; tp.disc_radius[1] = 0.75;
    tp.agent_pts = 4; tp.agent_stride = 13; tp.agent_flags = PO_AGENT_HOLD_BEFORE | PO_AGENT_HOLD_AFTER;
    const TrajectorySampler sampler(tp);
    const Trajectory r = sampler.sample(&engine, paths, t, ok);

    bool good = expect(r.status.size() == (size_t)B && r.samples.size() == (size_t)B && r.t.size() == (size_t)B && r.agents.size() == (size_t)B, "output sizes");
    uint64_t sum = 0, asum = 0;
    for (int b = 0; good && b < B; ++b) {
        const int st = r.status[b];
        good &= expect(r.samples[b].size() == (size_t)tp.K && r.t[b].size() == (size_t)tp.K && r.index[b].size() == (size_t)tp.K, "K samples per path");
        good &= expect(b == 4 ? st == 0 : st >= 1, "ok = 0 is not sampled, every other path is");
        good &= expect(r.agents[b].size() == (st == 0 ? 0u : 2u), "two agents per sampled path, none otherwise");
        good &= expect(b != 2 || st == 2, "the stopped path is held at rest");
        good &= expect(st == 0 ? r.first_held[b] == -1 : (r.first_held[b] >= 0 && r.first_held[b] <= tp.K && (st == 1) == (r.first_held[b] == tp.K)), "first_held follows the status");
        for (int k = 0; good && k < tp.K; ++k) {
            const State &s = r.samples[b][k];
            good &= expect(st == 0 ? (r.index[b][k] == -1 && r.t[b][k] == 0.0) : (r.index[b][k] >= 0 && r.index[b][k] < (int)paths[b].size()), "index names a state of the path");
            good &= expect(k == 0 || s.s >= r.samples[b][k - 1].s, "s never decreases along the samples");
            good &= expect(st == 0 || r.t[b][k] == tp.t0 + k * tp.dt, "the sample times");
            if (st != 0 && k >= r.first_held[b]) {
                const State &e = paths[b][r.index[b][k]];
                good &= expect(s.x == e.x && s.y == e.y && s.z == e.z && s.s == e.s && s.v == e.v && s.a == 0.0, "a held sample is a state of the path");
            }
            sum += bits(s.x) + bits(s.y) + bits(s.z) + bits(s.k) + bits(s.s) + bits(s.v) + bits(r.t[b][k]);
        }
        for (const Agent &a : r.agents[b]) {
            good &= expect(a.t.size() == 4 && a.hold_before && a.hold_after && a.t[3] == tp.t0 + 39 * tp.dt, "four points, the last one at the last sample");
            asum += bits(a.radius) + 4 + 3;  // n_pts + flags
            for (size_t j = 0; j < a.t.size(); ++j) asum += bits(a.t[j]) + bits(a.x[j]) + bits(a.y[j]);
        }
    }
    // the agents of path 5 as the set path 1 meets: DynamicChecker takes them as they are
    if (good) {
        std::vector<std::vector<Agent>> sets(1, r.agents[5]);
        const DynamicResult d = DynamicChecker().check(&engine, {paths[1]}, {t[1]}, sets);
        good &= expect(d.status.size() == 1 && d.status[0] >= 1, "the emitted agents are a valid set for DynamicChecker");
    }
    std::printf("status");
    for (int v : r.status) std::printf(" %d", v);
    std::printf("\nfirst_held");
    for (int v : r.first_held) std::printf(" %d", v);
    std::printf("\nchecksum %llu\nagents %llu\n", (unsigned long long)sum, (unsigned long long)asum);
    std::printf("%s\n", good ? "trajectory_test passed" : "trajectory_test FAILED");
    return good ? 0 : 1;
}
