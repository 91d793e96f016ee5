// The static world through the host mirror (map_tools.hpp): Ring::solid / Ring::free, World and MapStack::fromScene.  Two layers of 33 x 33 cells of 0.25 m around
// (0, 0) — every cell centre is a multiple of 0.25, so containment is exact — are built from rings and read back through the distance layers: a cell is occupied
// exactly when its distance is 0.  Checked: the lattice counts of the L ring (48), the square ring (64, low edges in, high edges out) and the free square
// (1089 - 64 occupied), a world window, a scene without rings and world against MapStack::fromObstacles.  Exit code 0 = passed.
#include <cstdio>
#include <utility>
#include <vector>

#include "path_optimizer_amd/map_tools.hpp"

using namespace PathOptimizationNS;

namespace {
const int kS = 33;
const double kRes = 0.25;

int occupied_cells(const MapStack &st, int layer) {
    int n = 0;
    for (int j = 0; j < kS; ++j)
        for (int i = 0; i < kS; ++i) n += st.getObstacleDistance(layer, 4.0 - kRes * i, 4.0 - kRes * j) == 0.0;
    return n;
}
bool expect(bool ok, const char *what) {
    if (!ok) std::printf("FAILED: %s\n", what);
    return ok;
}
}  // namespace

int main() {
    typedef std::vector<std::pair<double, double>> Verts;
    const Verts l_ring = {{0, 0}, {2, 0}, {2, 1}, {1, 1}, {1, 2}, {0, 2}}, square = {{-1, -1}, {1, -1}, {1, 1}, {-1, 1}};
    const std::vector<std::vector<Obstacle>> none(2);
    const std::vector<double> pos(4, 0.0);
    bool ok = true;

    // layer 0: the L, solid; layer 1: the square, solid
    MapStack solid = MapStack::fromScene(none, {}, {{Ring::solid(l_ring)}, {Ring::solid(square)}}, false, kS, kS, kRes, pos);
    ok &= expect(occupied_cells(solid, 0) == 48, "the L ring contains 48 cell centres");
    ok &= expect(occupied_cells(solid, 1) == 64, "the square ring contains 64 cell centres");
    ok &= expect(solid.getObstacleDistance(1, -1.0, -1.0) == 0.0 && solid.getObstacleDistance(1, 1.0, 1.0) > 0.0, "low edges in, high edges out");

    // the square as the only free ring of both layers (shared); layer 1 also owns a solid island inside it
    const Verts island = {{-0.5, -0.5}, {0.0, -0.5}, {0.0, 0.0}, {-0.5, 0.0}};
    MapStack free_sq = MapStack::fromScene(none, {Ring::free(square)}, {{}, {Ring::solid(island)}}, false, kS, kS, kRes, pos);
    ok &= expect(occupied_cells(free_sq, 0) == kS * kS - 64, "a free square leaves 1025 occupied cells");
    ok &= expect(occupied_cells(free_sq, 1) == kS * kS - 64 + 4, "a solid island inside a free ring is occupied");

    // a world of 4 x 4 cells of 1 m around (0, 0) whose cell (0, 0) — the corner at the largest x and y — is occupied; outside the world is occupied too
    std::vector<unsigned char> world(16, 255);
    world[0] = 0;
    World w(world.data(), 4, 4, 1.0, 0.0, 0.0, true);
    ok &= expect(w.cells() == 16, "world_cells");
    MapStack windowed = MapStack::fromScene(none, {}, {}, true, kS, kS, kRes, pos);
    // centres with -2 < x, y <= 2 lie inside the world (isInside is half open: 16 per axis); the occupied world cell holds those with 1 < x, y <= 2
    ok &= expect(occupied_cells(windowed, 0) == kS * kS - 16 * 16 + 4 * 4, "the world window");
    w.clear();
    ok &= expect(w.cells() == 0, "world cleared");

    // without rings and without world a scene is fromObstacles
    const std::vector<std::vector<Obstacle>> discs = {{Obstacle::disc(0.5, -0.5, 1.25)}, {Obstacle::box(-1.0, 1.0, 1.0, 0.5, 0.3)}};
    MapStack a = MapStack::fromScene(discs, {}, {}, false, kS, kS, kRes, pos);
    std::vector<double> da, db;
    for (int k = 0; k < 2; ++k)
        for (int j = 0; j < kS; ++j)
            for (int i = 0; i < kS; ++i) da.push_back(a.getObstacleDistance(k, 4.0 - kRes * i, 4.0 - kRes * j));
    MapStack b = MapStack::fromObstacles(discs, kS, kS, kRes, pos);
    for (int k = 0; k < 2; ++k)
        for (int j = 0; j < kS; ++j)
            for (int i = 0; i < kS; ++i) db.push_back(b.getObstacleDistance(k, 4.0 - kRes * i, 4.0 - kRes * j));
    ok &= expect(da == db, "a scene without rings and world equals fromObstacles");

    std::printf(ok ? "scene_test passed\n" : "scene_test FAILED\n");
    return ok ? 0 : 1;
}
