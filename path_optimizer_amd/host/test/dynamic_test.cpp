// Moving obstacles through the host mirror (dynamic_check.hpp): DynamicChecker::check on a small seeded case — 7 paths of 2 .. 35 states (0.5 m and 0.25 s apart),
// three agent sets (five agents of 1 .. 8 points, none, five), a set per path, one path with ok = 0, limits of 6 m/s on every other path.  Every number comes from
// an integer generator and dyadic arithmetic, so tests/test_dynamic.py rebuilds the same case bit for bit and compares the statuses and the checksum of gap printed
// here with Engine.dynamic_batch and the reference.  No map is set: the stage reads none.  Checked here: the shapes, that a path of the empty set is free, that
// v_limit is 0 exactly from the stop state on, and that the first conflict lies below the margin.  Exit code 0 = passed.
#include <cfloat>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "path_optimizer_amd/dynamic_check.hpp"

using namespace PathOptimizationNS;

namespace {
unsigned lcg_state = 13579u;
double u() {  // a multiple of 1 / 64 in [-2, 2]
    lcg_state = (lcg_state * 1103515245u + 12345u) & 0x7fffffffu;
    return ((int)((lcg_state >> 8) % 257u) - 128) / 64.0;
}
bool expect(bool ok, const char *what) {
    if (!ok) std::printf("FAILED: %s\n", what);
    return ok;
}
}  // namespace

int main() {
    const int B = 7;
    PoEngine engine(0);
    std::vector<std::vector<State>> paths(B);
    std::vector<std::vector<double>> t(B);
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < 2 + (b * 11) % 41; ++i) {
            const double x = -12.0 + 0.5 * i + u() / 8, y = u(), z = u() / 4, k = u() / 8;
            paths[b].emplace_back(x, y, z, k, 0.5 * i);
            t[b].push_back(0.25 * i);
        }
    std::vector<std::vector<Agent>> sets(3);
    for (int s = 0; s < 3; ++s)
        for (int a = 0; a < (s == 1 ? 0 : 5); ++a) {
            const int npts = 1 + (a * 3 + s) % 8, flags = (a + s) % 4;
            const double t0 = u(), x0 = 4 * u(), y0 = u();
            Agent g(0.25 + 0.125 * a, (flags & 1) != 0, (flags & 2) != 0);
            for (int j = 0; j < npts; ++j) g.add(t0 + 0.75 * j, x0 + 0.5 * j, y0 + (j % 2) * 0.25);
            sets[s].push_back(g);
        }
    std::vector<int> set_of(B), ok(B, 1);
    for (int b = 0; b < B; ++b) set_of[b] = b % 3;
    ok[5] = 0;
    std::vector<std::vector<double>> v_limit_in(B);
    for (int b = 0; b < B; b += 2) v_limit_in[b].assign(paths[b].size(), 6.0);

    DynamicParams dp;
    dp.stop_distance = 1.0;
    const DynamicResult r = DynamicChecker(dp).check(&engine, paths, t, sets, set_of, ok, v_limit_in);

    bool good = expect(r.status.size() == (size_t)B && r.gap.size() == (size_t)B && r.v_limit.size() == (size_t)B, "output sizes");
    uint64_t sum = 0;
    for (int b = 0; good && b < B; ++b) {
        const size_t n = paths[b].size();
        good &= expect(r.gap[b].size() == n && r.v_limit[b].size() == n, "one gap and one limit per state");
        good &= expect(b == 5 ? r.status[b] == 0 : r.status[b] >= 1, "ok = 0 is not checked, every other path is");
        good &= expect(set_of[b] != 1 || b == 5 || (r.status[b] == 1 && r.gap_min[b] == DBL_MAX), "a path of the empty set is free");
        const double open = b % 2 ? -1.0 : 6.0;
        for (size_t i = 0; good && i < n; ++i) {
            const bool stopped = r.status[b] >= 2 && (int)i >= r.stop_state[b];
            good &= expect(r.v_limit[b][i] == (stopped ? 0.0 : open), "v_limit is 0 exactly from the stop state on");
            uint64_t bits;
            std::memcpy(&bits, &r.gap[b][i], sizeof bits);
            sum += bits;
        }
        if (good && r.status[b] >= 2) {
            const int f = r.first_state[b];
            good &= expect(f >= 0 && r.stop_state[b] <= f && r.gap[b][f] < dp.margin && r.first_time[b] == t[b][f], "the first conflict lies below the margin");
            good &= expect(r.first_agent[b] >= 0 && r.ok()[b] == 0, "a conflict names its agent and clears ok");
        }
    }
    std::printf("status");
    for (int v : r.status) std::printf(" %d", v);
    std::printf("\nchecksum %llu\n", (unsigned long long)sum);
    std::printf("%s\n", good ? "dynamic_test passed" : "dynamic_test FAILED");
    return good ? 0 : 1;
}
