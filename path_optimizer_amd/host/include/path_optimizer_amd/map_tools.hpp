// Host-side mirror of the reference's classes around the obstacle-distance map, backed by libpo_hip.so:
//
//   reference                                                          here
//   PathOptimizationNS::Map (include/path_optimizer/tools/Map.hpp)      Map: owns the layer "distance", uploads it to the engine once
//     getObstacleDistance(pos) / isInside(pos)  (src/tools/Map.cpp)       same names (device sampling, po_map_sample)
//   ReferencePath::updateBounds(const Map&)                             updateBounds(ReferencePath&, knots, map): po_bounds_batch
//     (-> ReferencePathImpl::updateBoundsImproved)                        fills the bounds and truncates the states like the reference
//   — new —                                                            MapStack: M layers of one geometry on the engine, each with its own centre,
//                                                                        and the instance -> layer table of the batched calls (po_set_map_stack*,
//                                                                        po_set_map_assignment)
//   — new —                                                            Obstacle::disc / box / polygon and MapStack::fromObstacles: the stack from per-layer
//                                                                        obstacle lists over an optional static grid, rasterised on the device
//                                                                        (po_set_map_stack_obstacles)
//   — new —                                                            Ring::solid / free, World and MapStack::fromScene: the static world — polygon rings of
//                                                                        any shape (drivable area, footprints) and the site's static grid, which each
//                                                                        layer windows at its own centre (po_set_world_occupancy, po_set_map_stack_scene;
//                                                                        DESIGN.md section 21)
//   CollisionChecker::isSingleStateCollisionFreeImproved(State)         same name; checkPaths(): the batched tail of optimizePath
//     (src/tools/collision_checker.cpp)                                   (po_postcheck_batch)
//
// The reference builds its Map from a grid_map::GridMap; here the caller hands over that layer's raw buffer
// (gm["distance"].data(), gm.getSize(), gm.getResolution(), gm.getPosition()) — or, second constructor, the OCCUPANCY buffer the reference's callers already
// compute as `binary` (gm["obstacle"] cast to unsigned char, 0 = occupied): the distance transform then runs on the device — see INTEGRATION.md §C.
#pragma once
#include <cmath>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "po_hip.h"
#include "data_struct.hpp"
#include "solver.hpp"

namespace PathOptimizationNS {

class Map {
 public:
    Map(const float *distance_col_major, int size_x, int size_y, double resolution, double pos_x, double pos_y, PoEngine *engine = nullptr)
        : engine_(engine ? engine : &PoEngine::instance()) {
        po_map m{distance_col_major, size_x, size_y, resolution, pos_x, pos_y};
        const int rc = po_set_map(engine_->handle(), &m);
        if (rc != PO_OK) throw std::runtime_error(std::string("po_set_map: ") + po_strerror(rc));
    }
    // From the occupancy image (Eigen::Matrix<unsigned char, Dynamic, Dynamic>, column-major like the float layer; 0 = occupied): replaces
    // cv::distanceTransform(binary, distance, CV_DIST_L2, CV_DIST_MASK_PRECISE) and `distance *= resolution` with po_set_map_occupancy (exact, on the device).
    Map(const unsigned char *occupancy_col_major, int size_x, int size_y, double resolution, double pos_x, double pos_y, PoEngine *engine = nullptr)
        : engine_(engine ? engine : &PoEngine::instance()) {
        po_occupancy o{occupancy_col_major, size_x, size_y, resolution, pos_x, pos_y};
        const int rc = po_set_map_occupancy(engine_->handle(), &o);
        if (rc != PO_OK) throw std::runtime_error(std::string("po_set_map_occupancy: ") + po_strerror(rc));
    }
    double getObstacleDistance(double x, double y) const { double d; int in; sample(x, y, &d, &in); return d; }
    bool isInside(double x, double y) const { double d; int in; sample(x, y, &d, &in); return in != 0; }
    PoEngine *engine() const { return engine_; }
 private:
    void sample(double x, double y, double *d, int *in) const {
        const double xy[2] = {x, y};
        if (po_map_sample(engine_->handle(), 1, xy, d, in) != PO_OK) throw std::runtime_error("po_map_sample failed");
    }
    PoEngine *engine_;
};

// One detected object of a layer's obstacle list (po_obstacle): a disc or a convex polygon with 3 .. 8 vertices, world frame.
struct Obstacle {
    po_obstacle o;
    static Obstacle disc(double x, double y, double radius) {
        Obstacle r{};
        r.o.kind = PO_OBS_DISC;
        r.o.v[0] = x; r.o.v[1] = y; r.o.v[2] = radius;
        return r;
    }
    // vertices (x, y) in order, either orientation
    static Obstacle polygon(const std::vector<std::pair<double, double>> &vertices) {
        if (vertices.size() < 3 || vertices.size() > PO_OBS_MAX_VERTS) throw std::invalid_argument("Obstacle::polygon: 3 .. 8 vertices");
        Obstacle r{};
        r.o.kind = PO_OBS_POLY;
        r.o.n_verts = (int)vertices.size();
        for (size_t i = 0; i < vertices.size(); ++i) { r.o.v[2 * i] = vertices[i].first; r.o.v[2 * i + 1] = vertices[i].second; }
        return r;
    }
    // An oriented box as a 4-vertex polygon: the corners are computed here, on the host — the device sees polygons only, no trigonometry enters the exact path.
    static Obstacle box(double cx, double cy, double half_length, double half_width, double yaw) {
        const double c = std::cos(yaw), s = std::sin(yaw);
        const int sl[4] = {1, -1, -1, 1}, sw[4] = {1, 1, -1, -1};
        std::vector<std::pair<double, double>> v;
        for (int i = 0; i < 4; ++i) v.emplace_back(cx + sl[i] * half_length * c - sw[i] * half_width * s, cy + sl[i] * half_length * s + sw[i] * half_width * c);
        return polygon(v);
    }
};

// A polygon ring of any shape with 3 .. PO_RING_MAX_VERTS vertices (x, y), world frame, either orientation, filled by the even-odd rule.  solid: its interior is
// occupied (a building footprint, a clustered obstacle).  free: free space (a drivable-area boundary) — a layer that owns free rings is occupied wherever none of
// them contains the cell.
struct Ring {
    std::vector<std::pair<double, double>> vertices;
    int flag;
    static Ring solid(std::vector<std::pair<double, double>> v) { return make(std::move(v), PO_RING_SOLID); }
    static Ring free(std::vector<std::pair<double, double>> v) { return make(std::move(v), PO_RING_FREE); }
 private:
    static Ring make(std::vector<std::pair<double, double>> v, int flag) {
        if (v.size() < 3 || v.size() > PO_RING_MAX_VERTS) throw std::invalid_argument("Ring: 3 .. 4096 vertices");
        return Ring{std::move(v), flag};
    }
};

// The site's static occupancy grid on the engine ([size_y][size_x] bytes, x contiguous, 0 = occupied; its own resolution and centre), kept until replaced or
// cleared.  Every MapStack::fromScene(..., use_world = true) on that engine reads it: each layer is a window into it at the layer's own centre.
class World {
 public:
    World(const unsigned char *occupancy, int size_x, int size_y, double resolution, double pos_x, double pos_y, bool outside_occupied, PoEngine *engine = nullptr)
        : engine_(engine ? engine : &PoEngine::instance()) {
        po_occupancy o{occupancy, size_x, size_y, resolution, pos_x, pos_y};
        const int rc = po_set_world_occupancy(engine_->handle(), &o, outside_occupied ? 1 : 0);
        if (rc != PO_OK) throw std::runtime_error(std::string("po_set_world_occupancy: ") + po_strerror(rc));
    }
    void clear() const { (void)po_set_world_occupancy(engine_->handle(), nullptr, 0); }
    long long cells() const { long long n = 0; (void)po_debug_get(engine_->handle(), "world_cells", &n); return n; }
    PoEngine *engine() const { return engine_; }
 private:
    PoEngine *engine_;
};

// M obstacle-distance layers of one size and resolution on one engine: one local grid per vehicle, per perception hypothesis, per scene.  Layer k is centred at
// pos_xy[2k], pos_xy[2k + 1].  Which layer instance b of a batched call reads is the engine's assignment (setAssignment); without one every instance reads layer 0.
// Installing a MapStack replaces the engine's Map and the other way round (an engine holds one stack; a Map is a stack of one).
class MapStack {
 public:
    // layers: [M][size_y][size_x] floats, every layer column-major like Map's
    MapStack(const float *layers, int M, int size_x, int size_y, double resolution, const std::vector<double> &pos_xy, PoEngine *engine = nullptr)
        : engine_(engine ? engine : &PoEngine::instance()), M_(M) {
        if (pos_xy.size() != 2 * (size_t)(M > 0 ? M : 0)) throw std::invalid_argument("MapStack: pos_xy must hold M (x, y) pairs");
        po_map m{layers, size_x, size_y, resolution, 0.0, 0.0};
        const int rc = po_set_map_stack(engine_->handle(), M, &m, pos_xy.data());
        if (rc != PO_OK) throw std::runtime_error(std::string("po_set_map_stack: ") + po_strerror(rc));
    }
    // occupancy: [M][size_y][size_x] bytes, 0 = occupied; the distance transform of all M images runs on the device (po_set_map_stack_occupancy)
    MapStack(const unsigned char *occupancy, int M, int size_x, int size_y, double resolution, const std::vector<double> &pos_xy, PoEngine *engine = nullptr)
        : engine_(engine ? engine : &PoEngine::instance()), M_(M) {
        if (pos_xy.size() != 2 * (size_t)(M > 0 ? M : 0)) throw std::invalid_argument("MapStack: pos_xy must hold M (x, y) pairs");
        po_occupancy o{occupancy, size_x, size_y, resolution, 0.0, 0.0};
        const int rc = po_set_map_stack_occupancy(engine_->handle(), M, &o, pos_xy.data());
        if (rc != PO_OK) throw std::runtime_error(std::string("po_set_map_stack_occupancy: ") + po_strerror(rc));
    }
    // One list of obstacles per layer over an optional static grid (base: nullptr, or [size_y][size_x] bytes shared by every layer, 0 = occupied): rasterised and
    // transformed on the device; only the lists and the base travel (po_set_map_stack_obstacles).
    static MapStack fromObstacles(const std::vector<std::vector<Obstacle>> &layers, int size_x, int size_y, double resolution, const std::vector<double> &pos_xy,
                                  const unsigned char *base = nullptr, PoEngine *engine = nullptr) {
        const int M = (int)layers.size();
        if (pos_xy.size() != 2 * (size_t)M) throw std::invalid_argument("MapStack: pos_xy must hold M (x, y) pairs");
        std::vector<po_obstacle> obs;
        std::vector<int> first(1, 0);
        for (const auto &l : layers) {
            for (const auto &ob : l) obs.push_back(ob.o);
            first.push_back((int)obs.size());
        }
        po_obstacle_lists ls{obs.data(), first.data(), (int)obs.size(), base, base ? 1 : 0, size_x, size_y, resolution, 0.0, 0.0};
        MapStack st(engine ? engine : &PoEngine::instance(), M);
        const int rc = po_set_map_stack_obstacles(st.engine_->handle(), M, &ls, pos_xy.data());
        if (rc != PO_OK) throw std::runtime_error(std::string("po_set_map_stack_obstacles: ") + po_strerror(rc));
        return st;
    }
    // fromObstacles plus the static world: `shared` rings belong to every layer, rings[k] to layer k alone (empty vector: no layer has rings of its own); with
    // use_world the engine's World contributes (po_set_map_stack_scene).
    static MapStack fromScene(const std::vector<std::vector<Obstacle>> &layers, const std::vector<Ring> &shared, const std::vector<std::vector<Ring>> &rings,
                              bool use_world, int size_x, int size_y, double resolution, const std::vector<double> &pos_xy, const unsigned char *base = nullptr,
                              PoEngine *engine = nullptr) {
        const int M = (int)layers.size();
        if (pos_xy.size() != 2 * (size_t)M) throw std::invalid_argument("MapStack: pos_xy must hold M (x, y) pairs");
        if (!rings.empty() && rings.size() != (size_t)M) throw std::invalid_argument("MapStack: rings must be empty or hold one list per layer");
        std::vector<po_obstacle> obs;
        std::vector<int> first(1, 0);
        for (const auto &l : layers) {
            for (const auto &ob : l) obs.push_back(ob.o);
            first.push_back((int)obs.size());
        }
        std::vector<double> verts;
        std::vector<int> start(1, 0), flags, rfirst;
        const auto add = [&](const Ring &r) {
            for (const auto &v : r.vertices) { verts.push_back(v.first); verts.push_back(v.second); }
            start.push_back((int)(verts.size() / 2));
            flags.push_back(r.flag);
        };
        for (const Ring &r : shared) add(r);
        if (!rings.empty()) {
            rfirst.push_back((int)flags.size());
            for (const auto &l : rings) {
                for (const Ring &r : l) add(r);
                rfirst.push_back((int)flags.size());
            }
        }
        po_scene sc{};
        sc.lists = po_obstacle_lists{obs.data(), first.data(), (int)obs.size(), base, base ? 1 : 0, size_x, size_y, resolution, 0.0, 0.0};
        sc.rings = po_rings{verts.data(), start.data(), flags.data(), (int)flags.size(), (int)(verts.size() / 2), (int)shared.size(), rfirst.empty() ? nullptr : rfirst.data()};
        sc.use_world = use_world ? 1 : 0;
        MapStack st(engine ? engine : &PoEngine::instance(), M);
        const int rc = po_set_map_stack_scene(st.engine_->handle(), M, &sc, pos_xy.data());
        if (rc != PO_OK) throw std::runtime_error(std::string("po_set_map_stack_scene: ") + po_strerror(rc));
        return st;
    }
    // layer_of[b] = the layer instance b reads; an index outside [0, M) throws and leaves the previous table in force.  Empty: every instance reads layer 0.
    void setAssignment(const std::vector<int> &layer_of) const {
        const int rc = po_set_map_assignment(engine_->handle(), (int)layer_of.size(), layer_of.empty() ? nullptr : layer_of.data());
        if (rc != PO_OK) throw std::invalid_argument(std::string("po_set_map_assignment: ") + po_strerror(rc));
    }
    double getObstacleDistance(int layer, double x, double y) const { double d; int in; sample(layer, x, y, &d, &in); return d; }
    bool isInside(int layer, double x, double y) const { double d; int in; sample(layer, x, y, &d, &in); return in != 0; }
    int layers() const { return M_; }
    PoEngine *engine() const { return engine_; }
 private:
    MapStack(PoEngine *engine, int M) : engine_(engine), M_(M) {}
    void sample(int layer, double x, double y, double *d, int *in) const {
        const double xy[2] = {x, y};
        if (po_map_sample_layer(engine_->handle(), layer, 1, xy, d, in) != PO_OK) throw std::runtime_error("po_map_sample_layer failed");
    }
    PoEngine *engine_;
    int M_;
};

// The knots x_s_ / y_s_ were set from (tk::spline::set_points; ReferencePath::setSpline in the reference).
struct SplineKnots { std::vector<double> s, x, y; };

// ReferencePath::updateBounds for many reference paths at once.  Returns PO_OK or an API error code.
inline int updateBoundsBatch(ReferencePath *const *refs, const SplineKnots *const *knots, size_t B, const Map &map) {
    if (B == 0) return PO_OK;
    size_t N = 0, K = 0;
    for (size_t b = 0; b < B; ++b) { if (refs[b]->getSize() > N) N = refs[b]->getSize(); if (knots[b]->s.size() > K) K = knots[b]->s.size(); }
    if (N < 1 || K < 3) return PO_ERR_INVALID;
    std::vector<double> rx(B * N), ry(B * N), rz(B * N), rs(B * N), ks(B * K), kx(B * K), ky(B * K), bounds(B * N * 8);
    std::vector<int> npts(B), nk(B), nvalid(B);
    for (size_t b = 0; b < B; ++b) {
        const auto &st = refs[b]->getReferenceStates();
        npts[b] = (int)st.size(); nk[b] = (int)knots[b]->s.size();
        if (nk[b] < 3 || knots[b]->x.size() != knots[b]->s.size() || knots[b]->y.size() != knots[b]->s.size()) return PO_ERR_INVALID;
        for (size_t i = 0; i < st.size(); ++i) { rx[b * N + i] = st[i].x; ry[b * N + i] = st[i].y; rz[b * N + i] = st[i].z; rs[b * N + i] = st[i].s; }
        for (int i = 0; i < nk[b]; ++i) { ks[b * K + i] = knots[b]->s[i]; kx[b * K + i] = knots[b]->x[i]; ky[b * K + i] = knots[b]->y[i]; }
        for (size_t i = (size_t)nk[b]; i < K; ++i) ks[b * K + i] = ks[b * K + i - 1] + 1.0;  // padding stays increasing
    }
    po_bounds_in in{(int)B, (int)N, (int)K, rx.data(), ry.data(), rz.data(), rs.data(), npts.data(), ks.data(), kx.data(), ky.data(), nk.data()};
    const int rc = po_bounds_batch(map.engine()->handle(), &in, bounds.data(), nvalid.data());
    if (rc != PO_OK) return rc;
    for (size_t b = 0; b < B; ++b) {
        std::vector<CoveringCircleBounds> out((size_t)nvalid[b]);
        for (int i = 0; i < nvalid[b]; ++i) {
            CoveringCircleBounds::SingleCircleBounds *c[4] = {&out[i].c0, &out[i].c1, &out[i].c2, &out[i].c3};
            for (int j = 0; j < 4; ++j) { c[j]->lb = bounds[((b * N + i) * 4 + j) * 2]; c[j]->ub = bounds[((b * N + i) * 4 + j) * 2 + 1]; }
        }
        std::vector<State> st = refs[b]->getReferenceStates();
        st.resize((size_t)nvalid[b]);  // reference_path_impl.cpp:198-200
        refs[b]->setReference(std::move(st));
        refs[b]->setBounds(std::move(out));
    }
    return PO_OK;
}
inline void updateBounds(ReferencePath &ref, const SplineKnots &knots, const Map &map) {
    ReferencePath *r = &ref; const SplineKnots *k = &knots;
    const int rc = updateBoundsBatch(&r, &k, 1, map);
    if (rc != PO_OK) throw std::runtime_error(std::string("po_bounds_batch: ") + po_strerror(rc));
}

class CollisionChecker {
 public:
    explicit CollisionChecker(const Map &map) : map_(map) {}
    bool isSingleStateCollisionFreeImproved(const State &current) const {
        const double st[5] = {current.x, current.y, current.z, current.k, 0.0};
        po_info info{}; info.status = PO_STATUS_SOLVED;
        int nv = 0, ok = 0;
        if (po_postcheck_batch(map_.engine()->handle(), 1, 1, nullptr, st, &info, &nv, &ok) != PO_OK) throw std::runtime_error("po_postcheck_batch failed");
        return nv == 1;
    }
    // The tail of optimizePath (path_optimizer.cpp:183-200) for a batch of solved paths: truncates each path at its first colliding
    // state and returns, per path, what optimizePath returns.
    std::vector<bool> checkPaths(std::vector<std::vector<State>> *paths, const std::vector<po_info> &info) const {
        const size_t B = paths->size();
        size_t N = 1;
        for (auto &p : *paths) if (p.size() > N) N = p.size();
        std::vector<double> st(B * N * 5, 0.0);
        std::vector<int> npts(B), nv(B), ok(B);
        for (size_t b = 0; b < B; ++b) {
            npts[b] = (int)(*paths)[b].size();
            for (size_t i = 0; i < (*paths)[b].size(); ++i) {
                const State &s = (*paths)[b][i];
                double *o = &st[(b * N + i) * 5];
                o[0] = s.x; o[1] = s.y; o[2] = s.z; o[3] = s.k; o[4] = s.s;
            }
        }
        std::vector<bool> out(B, false);
        if (B == 0) return out;
        if (po_postcheck_batch(map_.engine()->handle(), (int)B, (int)N, npts.data(), st.data(), info.data(), nv.data(), ok.data()) != PO_OK)
            throw std::runtime_error("po_postcheck_batch failed");
        for (size_t b = 0; b < B; ++b) { (*paths)[b].resize((size_t)nv[b]); out[b] = ok[b] != 0; }
        return out;
    }
 private:
    const Map &map_;
};

}  // namespace PathOptimizationNS
