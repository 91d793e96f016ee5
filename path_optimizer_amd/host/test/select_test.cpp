// Score and select through the host mirror (path_select.hpp): PathSelector::select on a small seeded case — 11 candidates of 5 .. 11 states in 4 groups of 3, 1, 4
// and 2 (the last candidate belongs to no group), goals, one candidate with ok = 0, previous paths of 4, 0, 2 and 6 points — on a 40 x 30 map of 0.5 m cells.
// Every number comes from an integer generator and dyadic arithmetic, so tests/test_select.py rebuilds the same case bit for bit and compares the indices printed
// here with Engine.select_batch.  Checked here: the winners are the rows of candidates[best[g]], costs and counts are consistent.  Exit code 0 = passed.
#include <cmath>
#include <cstdio>
#include <vector>

#include "path_optimizer_amd/map_tools.hpp"
#include "path_optimizer_amd/path_select.hpp"

using namespace PathOptimizationNS;

namespace {
unsigned lcg_state = 12345u;
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
    const int kSx = 40, kSy = 30, B = 11;
    const std::vector<int> group_sizes = {3, 1, 4, 2}, prev_len = {4, 0, 2, 6};
    std::vector<float> layer((size_t)kSx * kSy);
    for (int j = 0; j < kSy; ++j)
        for (int i = 0; i < kSx; ++i) layer[(size_t)j * kSx + i] = 0.125f * (float)((i * 7 + j * 13) % 23);
    Map map(layer.data(), kSx, kSy, 0.5, 0.0, 0.0);

    std::vector<std::vector<State>> candidates(B), previous(group_sizes.size());
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < 5 + (b * 3) % 7; ++i) {
            const double x = -6.0 + 0.5 * i + u() / 4, y = u() * 2, z = u() / 2, k = u() / 8;
            candidates[b].emplace_back(x, y, z, k, 0.5 * i);
        }
    for (size_t g = 0; g < previous.size(); ++g)
        for (int j = 0; j < prev_len[g]; ++j) {
            const double x = -6.0 + 1.0 * j + u() / 4, y = u() * 2;
            previous[g].emplace_back(x, y);
        }
    std::vector<State> goals;
    for (int b = 0; b < B; ++b) { const double x = 4.0 + u(), y = u(); goals.emplace_back(x, y); }
    std::vector<int> ok(B, 1);
    ok[4] = 0;

    SelectParams sp;
    sp.min_clearance = -10.0;
    const Selection r = PathSelector(sp).select(map.engine(), candidates, group_sizes, ok, goals, previous);

    bool good = expect(r.best.size() == 4 && r.winners.size() == 4 && r.cost.size() == (size_t)B && r.feat.size() == (size_t)B * PO_N_FEAT, "output sizes");
    int first = 0;
    for (size_t g = 0; good && g < r.best.size(); ++g) {
        const int bb = r.best[g];
        good &= expect(bb >= first && bb < first + group_sizes[g], "the winner belongs to its group");
        int feasible = 0;
        for (int b = first; b < first + group_sizes[g]; ++b) {
            feasible += std::isfinite(r.cost[b]) ? 1 : 0;
            good &= expect(!(r.cost[b] < r.best_cost[g]), "no candidate of the group is cheaper than the winner");
        }
        good &= expect(feasible == r.n_feasible[g] && r.cost[bb] == r.best_cost[g], "counts and costs are consistent");
        good &= expect(r.winners[g].size() == candidates[bb].size(), "the winner's length");
        for (size_t i = 0; good && i < r.winners[g].size(); ++i) {
            const State &a = r.winners[g][i], &c = candidates[bb][i];
            good &= expect(a.x == c.x && a.y == c.y && a.z == c.z && a.k == c.k && a.s == c.s, "the winner's rows are the candidate's");
        }
        first += group_sizes[g];
    }
    good &= expect(!std::isfinite(r.cost[4]), "ok = 0 is infeasible");
    good &= expect(r.feat[(size_t)(B - 1) * PO_N_FEAT + PO_FEAT_DEV_PREV] == 0.0 && r.feat[3 * PO_N_FEAT + PO_FEAT_DEV_PREV] == 0.0,
                   "no deviation without a group or without a previous path");
    good &= expect(r.feat[0 * PO_N_FEAT + PO_FEAT_DEV_PREV] > 0.0 && r.feat[0 * PO_N_FEAT + PO_FEAT_GOAL] > 0.0, "deviation and goal distance are read");
    std::printf("best");
    for (int v : r.best) std::printf(" %d", v);
    std::printf("\nn_feasible");
    for (int v : r.n_feasible) std::printf(" %d", v);
    std::printf("\nsel_n");
    for (const auto &w : r.winners) std::printf(" %d", (int)w.size());
    std::printf("\n%s\n", good ? "select_test passed" : "select_test FAILED");
    return good ? 0 : 1;
}
