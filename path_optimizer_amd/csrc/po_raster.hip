// po_raster.hip — per-layer obstacle lists -> occupancy images on the device (gfx950): the step in front of po_edt.hip.  A planner holds one static grid and, per
// vehicle or perception hypothesis, a short list of detected objects (discs, convex polygons); this kernel turns M such lists into the M byte images
// po_launch_edt reads, so that the images never exist on the host.
//
// Definition (include/po_hip.h), evaluated in IEEE double, one rounding per operation (this object is compiled with -ffp-contract=off):
//     centre of cell (i, j) of layer k:  px = (pos_x[k] + (0.5 * (size_x * res) - 0.5 * res)) + res * (-i),  py likewise with size_y, pos_y[k], j
//     occupied  <=>  base cell == 0 (when a base is given)  or  some obstacle of the layer covers (px, py)
//     DISC  covers  <=>  dx = px - v[0], dy = py - v[1]:  dx * dx + dy * dy <= v[2] * v[2]
//     POLY  covers  <=>  (px, py) in the closed bounding box of the vertices (exact min / max)  and  the cross products
//                        (bx - ax) * (py - ay) - (by - ay) * (px - ax) of all edges (a -> b, the last edge closing) are all >= 0 or all <= 0
//     an unknown kind, a POLY with fewer than 3 vertices (n_verts is read clamped into [0, 8]) or a NaN among the values its kind reads: covers nothing
//     first[] is read clamped into [0, n_obs]: a bad list rasterises wrongly, it never reads outside obs
// Output: 0 = occupied, 255 = free, [M][size_y][size_x], x contiguous (po_occupancy's layout).
//
// Mapping.  One workgroup of 256 threads per (tile, layer), grid (tiles_x, tiles_y, M).  A tile is 64 cells along x by 16 rows; a thread owns four consecutive x cells
// of one row and writes them as one 4-byte store (bytes at the right edge).  Everything that depends on the layer alone (its centre, its slice of the list, its base
// image) is workgroup-uniform.
//   cull   the list is walked in rounds of kCap obstacles: lane t of the first wave takes obstacle t of the round, tests it against the tile and, when it may touch
//          the tile, appends it to a list in LDS (an LDS atomic on the counter: occupancy is an OR over the obstacles, their order cannot change it).
//   test   every thread runs its four cell centres against the LDS list (all lanes read the same LDS word: a broadcast) and leaves the loop once all four are occupied.
// A tile nothing touches runs no test at all and is a plain fill.
// The cull is CONSERVATIVE by monotonicity, not by a margin.  The computed cell centres are monotone in the index (every operation of the centre expression is
// monotone and rounding is monotone), so all centres of the tile lie in [xmin, xmax] x [ymin, ymax] taken from the tile's first and last cell, computed by the same
// expression.  POLY: the exact bounding box is part of the definition; a box that misses that rectangle contains no centre of the tile.  DISC: let q be the point of
// the rectangle nearest to the disc's centre (a clamp, exact).  For every centre p of the tile |p.x - v[0]| >= |q.x - v[0]| exactly, and subtraction, squaring and
// addition with rounding are monotone in those magnitudes, so the ROUNDED left-hand side at p is >= the rounded left-hand side at q: when q fails the predicate,
// every centre of the tile fails it.  No obstacle is dropped that the definition, which has no cull, would let cover a cell.
// No scratch, no dependence on launch order, no global atomics; plain C++ stores only.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "po_launch.hpp"

namespace {

constexpr int kTileX = 64;    // cells along x per tile
constexpr int kTileY = 16;    // rows per tile
constexpr int kCells = 4;     // consecutive x cells per thread
constexpr int kThreads = (kTileX / kCells) * kTileY;  // 256
constexpr int kCap = 64;      // obstacles per round (LDS list: 64 x 136 bytes + 64 boxes)

static_assert(sizeof(po_obstacle) == 136, "po_obstacle layout");

struct RasterArgs {
    const po_obstacle *obs;
    const int *first;
    int n_obs;
    const unsigned char *base;  // nullptr: no base
    size_t base_stride;         // 0: one image shared by every layer
    int sx, sy;
    double res, px, py;
    const double *pos_xy;       // [M][2] or nullptr
    unsigned char *out;
};

// getPositionFromIndex (csrc/po_map.hpp, map_position): p = (mapPos + (0.5 * len - 0.5 * res)) + res * (-idx), len = size * res.  A copy: this file shares no header
// with the map stages.
__device__ __forceinline__ double cell_origin(double pos, int size, double res) {
    return __dadd_rn(pos, __dsub_rn(__dmul_rn(0.5, __dmul_rn((double)size, res)), __dmul_rn(0.5, res)));
}
__device__ __forceinline__ double cell_centre(double origin, double res, int idx) { return __dadd_rn(origin, __dmul_rn(res, (double)(-idx))); }

__device__ __forceinline__ bool disc_covers(double px, double dy2, double cx, double r2) {
    const double dx = __dsub_rn(px, cx);
    return __dadd_rn(__dmul_rn(dx, dx), dy2) <= r2;
}

__global__ __launch_bounds__(kThreads) void raster_kernel(const RasterArgs a) {
    __shared__ po_obstacle s_obs[kCap];
    __shared__ double s_box[kCap][4];  // POLY: min x, max x, min y, max y
    __shared__ int s_count[2];

    const int t = threadIdx.x;
    const int k = blockIdx.z;
    const int i_lo = blockIdx.x * kTileX, j_lo = blockIdx.y * kTileY;
    const int i_hi = min(i_lo + kTileX - 1, a.sx - 1), j_hi = min(j_lo + kTileY - 1, a.sy - 1);
    const int i0 = i_lo + kCells * (t & (kTileX / kCells - 1)), j = j_lo + t / (kTileX / kCells);

    const double pos_x = a.pos_xy ? a.pos_xy[2 * (size_t)k] : a.px, pos_y = a.pos_xy ? a.pos_xy[2 * (size_t)k + 1] : a.py;
    const double ox = cell_origin(pos_x, a.sx, a.res), oy = cell_origin(pos_y, a.sy, a.res);
    // the tile's extent: index 0 is the LARGEST coordinate
    const double xmax = cell_centre(ox, a.res, i_lo), xmin = cell_centre(ox, a.res, i_hi);
    const double ymax = cell_centre(oy, a.res, j_lo), ymin = cell_centre(oy, a.res, j_hi);
    const double py = cell_centre(oy, a.res, j);
    double px[kCells];
#pragma unroll
    for (int c = 0; c < kCells; ++c) px[c] = cell_centre(ox, a.res, i0 + c);

    const int lo = min(max(a.first[k], 0), a.n_obs), hi = min(max(a.first[k + 1], 0), a.n_obs);
    bool occ[kCells] = {false, false, false, false};

    if (lo < hi) {
        if (t == 0) s_count[0] = 0;
        __syncthreads();
    }
    int round = 0;
    for (int r0 = lo; r0 < hi; r0 += kCap, ++round) {
        int *count = &s_count[round & 1];
        // ---- cull: one obstacle per lane of the first wave ----
        if (t == 0) s_count[(round + 1) & 1] = 0;  // (the next round's counter: last read before the barrier that ended the previous round)
        if (t < kCap && r0 + t < hi) {
            const po_obstacle o = a.obs[r0 + t];
            bool keep = false;
            double bx0 = 0, bx1 = 0, by0 = 0, by1 = 0;
            if (o.kind == PO_OBS_DISC) {
                const double cx = o.v[0], cy = o.v[1], r = o.v[2];
                if (cx == cx && cy == cy && r == r) {
                    const double qx = fmin(fmax(cx, xmin), xmax), qy = fmin(fmax(cy, ymin), ymax);  // nearest point of the tile's rectangle (exact)
                    const double dy = __dsub_rn(qy, cy);
                    keep = disc_covers(qx, __dmul_rn(dy, dy), cx, __dmul_rn(r, r));
                }
            } else if (o.kind == PO_OBS_POLY) {
                const int n = min(max(o.n_verts, 0), PO_OBS_MAX_VERTS);
                if (n >= 3) {
                    bool nan = false;
                    bx0 = bx1 = o.v[0];
                    by0 = by1 = o.v[1];
#pragma unroll  // (static indices: `o` lives in registers)
                    for (int e = 0; e < PO_OBS_MAX_VERTS; ++e) {
                        if (e < n) {
                            const double vx = o.v[2 * e], vy = o.v[2 * e + 1];
                            nan = nan || vx != vx || vy != vy;
                            bx0 = fmin(bx0, vx); bx1 = fmax(bx1, vx);
                            by0 = fmin(by0, vy); by1 = fmax(by1, vy);
                        }
                    }
                    keep = !nan && bx1 >= xmin && bx0 <= xmax && by1 >= ymin && by0 <= ymax;
                }
            }
            if (keep) {
                const int slot = atomicAdd(count, 1);  // LDS; at most kCap candidates per round, so slot < kCap
                s_obs[slot] = o;
                s_box[slot][0] = bx0; s_box[slot][1] = bx1; s_box[slot][2] = by0; s_box[slot][3] = by1;
            }
        }
        __syncthreads();
        // ---- test: four cell centres per thread against the survivors ----
        const int n_live = *count;
        for (int s = 0; s < n_live; ++s) {
            if (occ[0] && occ[1] && occ[2] && occ[3]) break;
            const po_obstacle &o = s_obs[s];
            if (o.kind == PO_OBS_DISC) {
                const double cx = o.v[0], cy = o.v[1], r = o.v[2];
                const double dy = __dsub_rn(py, cy), dy2 = __dmul_rn(dy, dy), r2 = __dmul_rn(r, r);
#pragma unroll
                for (int c = 0; c < kCells; ++c) occ[c] = occ[c] || disc_covers(px[c], dy2, cx, r2);
            } else {
                const int n = min(max(o.n_verts, 0), PO_OBS_MAX_VERTS);
                const bool in_y = py >= s_box[s][2] && py <= s_box[s][3];
                bool all_pos[kCells], all_neg[kCells];
#pragma unroll
                for (int c = 0; c < kCells; ++c) all_pos[c] = all_neg[c] = in_y && px[c] >= s_box[s][0] && px[c] <= s_box[s][1];
                double ax = o.v[2 * (n - 1)], ay = o.v[2 * (n - 1) + 1];  // the closing edge first: the result is an AND over the edges, their order cannot change it
                for (int e = 0; e < n; ++e) {
                    const double bx = o.v[2 * e], by = o.v[2 * e + 1];
                    const double ex = __dsub_rn(bx, ax), ey = __dsub_rn(by, ay);
                    const double ry = __dmul_rn(ex, __dsub_rn(py, ay));
#pragma unroll
                    for (int c = 0; c < kCells; ++c) {
                        const double cr = __dsub_rn(ry, __dmul_rn(ey, __dsub_rn(px[c], ax)));
                        all_pos[c] = all_pos[c] && cr >= 0.0;
                        all_neg[c] = all_neg[c] && cr <= 0.0;
                    }
                    ax = bx; ay = by;
                }
#pragma unroll
                for (int c = 0; c < kCells; ++c) occ[c] = occ[c] || all_pos[c] || all_neg[c];
            }
        }
        __syncthreads();  // the LDS list is rewritten by the next round
    }

    if (j >= a.sy || i0 >= a.sx) return;
    const size_t cell = (size_t)j * (size_t)a.sx + (size_t)i0;
    unsigned char *dst = a.out + (size_t)k * (size_t)a.sx * (size_t)a.sy + cell;
    const unsigned char *b = a.base ? a.base + (size_t)k * a.base_stride + cell : nullptr;
    if (i0 + kCells <= a.sx) {
        uint32_t free_mask = 0xFFFFFFFFu;
        if (b) {
            uint32_t w;
            __builtin_memcpy(&w, b, sizeof(w));  // (rows start at any byte address: an unaligned 4-byte access, which global memory serves)
#pragma unroll
            for (int c = 0; c < kCells; ++c)
                if (((w >> (8 * c)) & 0xFFu) == 0) free_mask &= ~(0xFFu << (8 * c));
        }
#pragma unroll
        for (int c = 0; c < kCells; ++c)
            if (occ[c]) free_mask &= ~(0xFFu << (8 * c));
        __builtin_memcpy(dst, &free_mask, sizeof(free_mask));
    } else {
        for (int c = 0; c < kCells && i0 + c < a.sx; ++c) dst[c] = (occ[c] || (b && b[c] == 0)) ? 0 : 255;
    }
}

}  // namespace

// Lists, base and pos_xy are device pointers; out [M][sy][sx].  The caller has checked 1 <= sx, sy <= po_edt_max_side(), 1 <= M <= po_edt_max_images() (grid.z),
// n_obs >= 0 and base_count in {0, 1, M}.
extern "C" hipError_t po_launch_raster(const po_obstacle_lists *L, int M, const double *pos_xy, unsigned char *out, hipStream_t st) {
    RasterArgs a{};
    a.obs = L->obs; a.first = L->first; a.n_obs = L->n_obs;
    a.base = L->base_count > 0 ? L->base : nullptr;
    a.base_stride = (L->base_count == M && M > 1) ? (size_t)L->size_x * (size_t)L->size_y : 0;
    a.sx = L->size_x; a.sy = L->size_y;
    a.res = L->resolution; a.px = L->pos_x; a.py = L->pos_y;
    a.pos_xy = pos_xy;
    a.out = out;
    const dim3 grid((a.sx + kTileX - 1) / kTileX, (a.sy + kTileY - 1) / kTileY, M);
    hipLaunchKernelGGL(raster_kernel, grid, dim3(kThreads), 0, st, a);
    return hipGetLastError();
}
