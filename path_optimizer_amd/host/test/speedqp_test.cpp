// The speed QP through the host mirror (speed_qp.hpp): SpeedQp::solve on three straight paths of 41 states 0.5 m apart with hand-built plans over windows of 1 s
// (drive through, wait a window then drive, drive and stand), two blocked cells beside the plans, 36 samples 0.125 s apart.  Every input is dyadic, so
// tests/test_speedqp.py (mirror_case) builds the same case bit for bit and compares the statuses, iteration counts, sample counts and the checksum of the samples
// printed here with Engine.speedqp_batch and the reference.  No map is set: the stage reads none.  Checked here: the shapes, that sample 0 is pinned at state 0 (to the solver's tolerance) with v0, that
// the times are q * dts, that every position lies in its tunnel within the primal threshold's order (1e-2 m), that the held samples repeat the last sample of the
// QP with a = jerk = 0, and that a path without a plan is not run.  Exit code 0 = passed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "path_optimizer_amd/speed_qp.hpp"

using namespace PathOptimizationNS;

namespace {
bool expect(bool ok, const char *what) {
    if (!ok) std::printf("FAILED: %s\n", what);
    return ok;
}
uint64_t bits_of(double v) {
    uint64_t b;
    std::memcpy(&b, &v, sizeof b);
    return b;
}
}  // namespace

int main() {
    const int B = 3, N = 41;
    PoEngine engine(0);
    SpeedQpParams qp;
    qp.dt = 1.0; qp.K = 4; qp.stride = 2; qp.v_max = 4.0; qp.dts = 0.125; qp.Q = 36; qp.max_iter = 200;
    const int Q = qp.Q;
    std::vector<std::vector<State>> paths(B);
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < N; ++i) paths[b].emplace_back(0.5 * i, 0.25 * b, 0.0, 0.0, 0.5 * i);
    const std::vector<double> v0 = {1.0, 0.5, 2.0};
    const std::vector<std::vector<int>> station = {{0, 1, 3, 5, 6}, {0, 0, 1, 3, 5}, {0, 2, 2}};
    std::vector<std::vector<double>> ref_s(B, std::vector<double>(Q));
    for (int b = 0; b < B; ++b) {
        const int nl = (int)station[b].size() - 1;
        for (int q = 0; q < Q; ++q) {
            const double t = q * qp.dts;
            int kk = 0;
            for (int k = 1; k <= nl; ++k)
                if (k * qp.dt <= t) kk = k;
            const double Sp = 1.0 * station[b][kk];  // stations are 1 m apart
            ref_s[b][q] = kk == nl ? Sp : Sp + (1.0 * station[b][kk + 1] - Sp) / qp.dt * (t - kk * qp.dt);
        }
    }
    std::vector<int> cells((size_t)B * qp.K * PO_ST_MAX_STATIONS, -1);
    cells[((size_t)0 * qp.K + 1) * PO_ST_MAX_STATIONS + 5] = 1;
    cells[((size_t)1 * qp.K + 2) * PO_ST_MAX_STATIONS + 4] = 1;

    const SpeedQpResult r = SpeedQp(qp).solve(&engine, paths, v0, station, ref_s, cells);
    bool good = expect(r.status.size() == (size_t)B && r.samples.size() == (size_t)B && r.jerk.size() == (size_t)B && r.lo.size() == (size_t)B, "output sizes");
    uint64_t sum = 0;
    for (int b = 0; good && b < B; ++b) {
        const int n = r.n_q[b];
        good &= expect((int)r.samples[b].size() == Q && (int)r.t[b].size() == Q && (int)r.index[b].size() == Q, "Q samples per path");
        good &= expect(r.status[b] == 1 || r.status[b] == 2, "every path has a plan and is run");
        good &= expect(n == (b == 2 ? 17 : 33), "n_q counts the samples up to n_layers * dt");
        const State &p0 = r.samples[b][0];
        good &= expect(r.index[b][0] == 0 && p0.v == v0[b] && std::fabs(p0.s) < 1e-2 && r.lo[b][0] == 0 && r.hi[b][0] == 0, "sample 0 is pinned at state 0 with v0");
        for (int q = 0; good && q < Q; ++q) {
            const State &p = r.samples[b][q];
            good &= expect(r.t[b][q] == q * qp.dts, "the sample times are q * dts");
            good &= expect(p.s >= r.lo[b][q] - 1e-2 && p.s <= r.hi[b][q] + 1e-2, "a position lies in its tunnel");
            good &= expect(r.index[b][q] >= 0 && r.index[b][q] < N - 1, "a sample is anchored at a state of its path");
            if (q >= n) good &= expect(p.s == r.samples[b][n - 1].s && p.v == r.samples[b][n - 1].v && p.a == 0 && r.jerk[b][q] == 0, "held samples repeat the last one");
        }
        for (int q = 0; q < Q; ++q) {
            const State &p = r.samples[b][q];
            sum += bits_of(p.x) + bits_of(p.y) + bits_of(p.z) + bits_of(p.k) + bits_of(p.s) + bits_of(p.v) + bits_of(p.a) + bits_of(r.jerk[b][q]);
        }
    }
    // a path without a plan is not run
    std::vector<std::vector<int>> none = station;
    none[1].clear();
    const SpeedQpResult z = SpeedQp(qp).solve(&engine, paths, v0, none, ref_s, cells);
    good &= expect(z.status[1] == 0 && z.n_q[1] == 0 && z.index[1][0] == -1 && z.samples[1][5].s == 0 && z.status[0] == r.status[0], "no plan: not run");
    std::printf("status");
    for (int v : r.status) std::printf(" %d", v);
    std::printf("\niters");
    for (int v : r.iters) std::printf(" %d", v);
    std::printf("\nn_q");
    for (int v : r.n_q) std::printf(" %d", v);
    std::printf("\nchecksum %llu\n", (unsigned long long)sum);
    std::printf("%s\n", good ? "speedqp_test passed" : "speedqp_test FAILED");
    return good ? 0 : 1;
}
