// MapStack (map_tools.hpp) and PathOptimizer::solveBatch over it: three local grids with their own centres and obstacles, six planning problems interleaved over
// them (problem b drives through layer b % 3).  Each problem must come out exactly — every double of every state — as it does from a Map that holds its layer alone,
// and the problems of layers 1 and 2 must come out differently when they are (wrongly) planned on layer 0.  Exit code 0 = passed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "path_optimizer_amd/path_optimizer.hpp"

using namespace PathOptimizationNS;

namespace {
const int kSx = 300, kSy = 260, kLayers = 3;
const double kRes = 0.2;

// layer k: centre (40 k, -25 k), one disc a few metres beside the straight reference that runs through the centre along x
void make_layer(int k, float *dist, double *pos) {
    pos[0] = 40.0 * k; pos[1] = -25.0 * k;
    const double ox = pos[0] + 4.0 * (k - 1), oy = pos[1] + (k == 1 ? -1.0 : 1.0) * (3.5 + 0.3 * k), orad = 1.0;
    for (int j = 0; j < kSy; ++j)
        for (int i = 0; i < kSx; ++i) {
            const double cx = pos[0] + 0.5 * kSx * kRes - (i + 0.5) * kRes, cy = pos[1] + 0.5 * kSy * kRes - (j + 0.5) * kRes;
            const double dd = std::sqrt((cx - ox) * (cx - ox) + (cy - oy) * (cy - oy)) - orad;
            dist[(size_t)j * kSx + i] = (float)(dd > 0 ? dd : 0);
        }
}

PlanningProblem make_problem(int b, const double *pos) {
    PlanningProblem p;
    const double y = pos[1] + 0.15 * (b / kLayers), x0 = pos[0] - 20.0;
    for (int i = 0; i < 14; ++i) p.reference_points.emplace_back(x0 + 3.0 * i, y + ((i & 1) ? 0.1 : -0.1) * (i > 0 && i < 13), 0.0);
    p.start_state = State(x0, y, 0.0, 0.0, 0.0);
    p.end_state = State(x0 + 39.0, y, 0.0, 0.0, 0.0);
    return p;
}

bool same_path(const std::vector<State> &a, const std::vector<State> &b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i) {
        const double u[5] = {a[i].x, a[i].y, a[i].z, a[i].k, a[i].s}, v[5] = {b[i].x, b[i].y, b[i].z, b[i].k, b[i].s};
        if (std::memcmp(u, v, sizeof(u)) != 0) return false;
    }
    return true;
}
}  // namespace

int main() {
    const size_t cells = (size_t)kSx * kSy;
    std::vector<float> layers(kLayers * cells);
    std::vector<double> pos(2 * kLayers);
    for (int k = 0; k < kLayers; ++k) make_layer(k, &layers[k * cells], &pos[2 * k]);
    const int B = 6;
    std::vector<PlanningProblem> problems;
    std::vector<int> layer_of;
    for (int b = 0; b < B; ++b) { problems.push_back(make_problem(b, &pos[2 * (b % kLayers)])); layer_of.push_back(b % kLayers); }

    // what each layer alone gives for ALL problems (a Map is a stack of one)
    std::vector<std::vector<std::vector<State>>> alone(kLayers);
    std::vector<std::vector<bool>> alone_ok(kLayers);
    for (int k = 0; k < kLayers; ++k) {
        Map one(&layers[k * cells], kSx, kSy, kRes, pos[2 * k], pos[2 * k + 1]);
        alone_ok[k] = PathOptimizer::solveBatch(problems.data(), problems.size(), one, &alone[k]);
    }

    MapStack stack(layers.data(), kLayers, kSx, kSy, kRes, pos);
    bool ok = stack.layers() == kLayers;
    for (int k = 0; k < kLayers; ++k) {  // the layer's own centre is inside it and 0.5 m beyond its edge is not
        ok = ok && stack.isInside(k, pos[2 * k], pos[2 * k + 1]) && !stack.isInside(k, pos[2 * k] + 0.5 * kSx * kRes + 0.5, pos[2 * k + 1]);
        ok = ok && stack.getObstacleDistance(k, pos[2 * k], pos[2 * k + 1]) > 0.0;
    }
    std::vector<std::vector<State>> paths;
    std::vector<int> stage;
    const std::vector<bool> got = PathOptimizer::solveBatch(problems.data(), problems.size(), stack, layer_of, &paths, &stage);
    int solved = 0, differs_from_layer0 = 0;
    for (int b = 0; b < B; ++b) {
        const int k = b % kLayers;
        const bool same = got[b] == alone_ok[k][b] && same_path(paths[b], alone[k][b]);
        std::printf("problem %d on layer %d: ok=%d states=%zu stage=%d %s\n", b, k, (int)got[b], paths[b].size(), stage[b], same ? "== its own map" : "DIFFERS from its own map");
        ok = ok && same;
        solved += got[b] ? 1 : 0;
        if (k != 0 && !(got[b] == alone_ok[0][b] && same_path(paths[b], alone[0][b]))) ++differs_from_layer0;
    }
    ok = ok && solved == B && differs_from_layer0 == 4;
    bool refused = false;  // a layer index outside the stack is refused and the table stays
    try { stack.setAssignment(std::vector<int>(B, kLayers)); } catch (const std::invalid_argument &) { refused = true; }
    std::vector<std::vector<State>> again;
    const std::vector<bool> got2 = PathOptimizer::solveBatch(problems.data(), problems.size(), stack, layer_of, &again);
    for (int b = 0; b < B; ++b) ok = ok && got2[b] == got[b] && same_path(again[b], paths[b]);
    std::printf("solved %d of %d, %d of 4 differ from layer 0, bad table refused=%d\n", solved, B, differs_from_layer0, (int)refused);
    if (!(ok && refused)) { std::printf("map stack FAILED\n"); return 1; }
    std::printf("map stack ok\n");
    return 0;
}
