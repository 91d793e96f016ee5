// po_scene.hip — the static world of the map stack on the device (gfx950): the handle's world grid and polygon rings, ORed into the occupancy images that
// po_raster.hip has written (base + discs + convex polygons), in front of po_edt.hip.
//
// Definition (include/po_hip.h), evaluated in IEEE double, one rounding per operation (this object is compiled with -ffp-contract=off).  The
// centre (px, py) of cell (i, j) of layer k is po_raster.hip's, the same expression.  This kernel adds three clauses to "occupied":
//     world        lx = wsx * wres:  tx = -((px - wpx) - 0.5 * lx), inside_x <=> tx >= 0 && tx < lx,  ix = (int)(-(((px - 0.5 * lx) - wpx) / wres)); y likewise.
//                  inside and 0 <= ix < wsx and 0 <= iy < wsy:  occupied <=> world[iy][ix] == 0;  otherwise occupied <=> outside_occupied
//     SOLID rings  some SOLID ring the layer owns contains the centre
//     FREE rings   the layer owns at least one FREE ring and none of them contains the centre
//     contains     even-odd: the number of edges a -> b (the last one closing) with  (ay > py) != (by > py)  and  right  is odd, where
//                  t = (bx - ax) * (py - ay) - (by - ay) * (px - ax),  right = (by > ay) ? (t > 0) : (t < 0)
//     the layer owns rings [0, n_shared) and [first[k], first[k+1]); everything is read clamped (start[] into [0, n_verts], n_shared and first[] into [0, n_rings]);
//     a ring with fewer than 3 vertices or an unknown flag is ignored, one with more than PO_RING_MAX_VERTS is read as its first PO_RING_MAX_VERTS vertices.
//     Both ring clauses are ORs over rings, so a ring a bad table hands to a layer twice changes nothing.
//
// Structure.  An OVERLAY over po_launch_raster's image, not a kernel that does everything: po_raster.hip stays byte for byte what it was, the base / DISC / POLY
// clauses cannot drift between two copies, and a scene without rings and without world launches nothing here — its bytes ARE po_rasterize_batch's.  The price is one
// more read of the image (and a write of the 4-byte groups that change).
//
// Mapping.  po_raster.hip's: one workgroup of 256 threads per (tile, layer), a tile is 64 cells along x by 16 rows, a thread owns four consecutive x cells of one row.
// Everything that depends on the layer alone (its centre, its ring ranges) is workgroup-uniform.
//   world   80 threads compute the world index of the tile's 64 columns and 16 rows once (-1: outside) into LDS; every thread then gathers one byte per cell.
//   rings   one ring at a time, its edges streamed through LDS in rounds of 256: thread t takes edge t of the round, culls it against the tile and appends a survivor
//           to a list in LDS (an LDS atomic on the counter: parity is a XOR over the edges, their order cannot change it).  Then every thread runs its four centres
//           against the survivors and carries one parity bit per cell across the rounds.  A tile no edge survives for costs nothing but the culls, and its parity
//           is 0 everywhere: wholly outside the ring (a SOLID ring changes nothing, a layer whose FREE rings all miss the tile gets a fill of zeros).
// The culls are EXACT with respect to the definition, which has none, by monotonicity and not by a margin (DESIGN.md section 21 has the full argument).  All centres
// of the tile lie in [xmin, xmax] x [ymin, ymax], computed by the same expression from the tile's first and last cell (the expression is monotone in the index).
//   y     an edge with ay > ymax and by > ymax has (ay > py) == (by > py) == true on every row; one with !(ay > ymin) and !(by > ymin) has both false: it never straddles.
//   left  an edge with ax <= xmin and bx <= xmin is never `right` on a row it straddles: for by > ay the factors satisfy fl(bx - ax) <= fl(px - ax) and
//         0 <= fl(py - ay) <= fl(by - ay), so the rounded first product is <= the rounded second one and t <= 0 (or t is a NaN); by < ay mirrors it.
//   An edge wholly RIGHT of the tile is NOT culled: geometrically it counts on every row it straddles, but rounding can turn two different exact products into equal
//   rounded ones (t == 0: not `right`), so that shortcut cannot be argued and is left out.  The y cull already leaves a tile only the edges that cross its 16 rows.
// No scratch, no dependence on launch order, no global atomics; plain C++ stores only.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "po_launch.hpp"

namespace {

constexpr int kTileX = 64;    // cells along x per tile
constexpr int kTileY = 16;    // rows per tile
constexpr int kCells = 4;     // consecutive x cells per thread
constexpr int kThreads = (kTileX / kCells) * kTileY;  // 256 = edges per round

struct SceneArgs {
    const double *verts;        // [n_verts][2]
    const int *start, *flags;   // [n_rings + 1], [n_rings]
    const int *first;           // [M + 1] or nullptr
    int n_rings, n_verts, n_shared;
    const unsigned char *world;  // nullptr: the world clause is off
    int wsx, wsy, outside;
    double wres, wpx, wpy;
    int sx, sy;
    double res, px, py;
    const double *pos_xy;       // [M][2] or nullptr
    unsigned char *img;         // [M][sy][sx]: read, ORed into, written back
};

// po_raster.hip's cell centre (getPositionFromIndex): the same expression, so the same bits
__device__ __forceinline__ double cell_origin(double pos, int size, double res) {
    return __dadd_rn(pos, __dsub_rn(__dmul_rn(0.5, __dmul_rn((double)size, res)), __dmul_rn(0.5, res)));
}
__device__ __forceinline__ double cell_centre(double origin, double res, int idx) { return __dadd_rn(origin, __dmul_rn(res, (double)(-idx))); }

// isInside + getIndexFromPosition along one axis (csrc/po_map.hpp: map_inside, map_index, map_index_ok): the world index of coordinate p, -1 when p is outside
__device__ __forceinline__ int world_index(double p, double wpos, int wsize, double wres) {
    const double len = __dmul_rn((double)wsize, wres), half = __dmul_rn(0.5, len);
    const double t = -(__dsub_rn(__dsub_rn(p, wpos), half));
    if (!(t >= 0.0 && t < len)) return -1;
    const int idx = (int)(-(__ddiv_rn(__dsub_rn(__dsub_rn(p, half), wpos), wres)));  // (p is inside: the quotient is within a cell of [0, wsize])
    return (idx >= 0 && idx < wsize) ? idx : -1;
}

__global__ __launch_bounds__(kThreads) void scene_overlay_kernel(const SceneArgs a) {
    __shared__ double s_edge[kThreads][4];  // ax, ay, bx, by of the round's survivors
    __shared__ int s_count[2];
    __shared__ int s_wx[kTileX], s_wy[kTileY];

    const int t = threadIdx.x;
    const int k = blockIdx.z;
    const int i_lo = blockIdx.x * kTileX, j_lo = blockIdx.y * kTileY;
    const int i_hi = min(i_lo + kTileX - 1, a.sx - 1), j_hi = min(j_lo + kTileY - 1, a.sy - 1);
    const int ci = kCells * (t & (kTileX / kCells - 1)), cj = t / (kTileX / kCells);  // the thread's first column and its row, within the tile
    const int i0 = i_lo + ci, j = j_lo + cj;

    const double pos_x = a.pos_xy ? a.pos_xy[2 * (size_t)k] : a.px, pos_y = a.pos_xy ? a.pos_xy[2 * (size_t)k + 1] : a.py;
    const double ox = cell_origin(pos_x, a.sx, a.res), oy = cell_origin(pos_y, a.sy, a.res);
    // the tile's extent: index 0 is the LARGEST coordinate
    const double xmin = cell_centre(ox, a.res, i_hi);
    const double ymax = cell_centre(oy, a.res, j_lo), ymin = cell_centre(oy, a.res, j_hi);
    const double py = cell_centre(oy, a.res, j);
    double px[kCells];
#pragma unroll
    for (int c = 0; c < kCells; ++c) px[c] = cell_centre(ox, a.res, i0 + c);

    unsigned occ = 0;  // bit c: cell c of the thread is occupied by a clause of this kernel

    // ---- world: the index of every column and row of the tile once, then one byte per cell ----
    if (a.world) {
        if (t < kTileX) s_wx[t] = world_index(cell_centre(ox, a.res, i_lo + t), a.wpx, a.wsx, a.wres);
        else if (t < kTileX + kTileY) s_wy[t - kTileX] = world_index(cell_centre(oy, a.res, j_lo + (t - kTileX)), a.wpy, a.wsy, a.wres);
        __syncthreads();
        const int wy = s_wy[cj];
#pragma unroll
        for (int c = 0; c < kCells; ++c) {
            const int wx = s_wx[ci + c];
            bool o = a.outside != 0;
            if (wx >= 0 && wy >= 0 && j < a.sy && i0 + c < a.sx) o = a.world[(size_t)wy * (size_t)a.wsx + (size_t)wx] == 0;  // (0 <= wx < wsx, 0 <= wy < wsy)
            if (o) occ |= 1u << c;
        }
    }

    // ---- rings: the shared ones, then the layer's own ----
    const int nr = a.n_rings;
    const int n_sh = min(max(a.n_shared, 0), nr);
    const int own_lo = a.first ? min(max(a.first[k], 0), nr) : 0, own_hi = a.first ? min(max(a.first[k + 1], 0), nr) : 0;
    const int n_own = max(own_hi - own_lo, 0);
    bool has_free = false;
    unsigned in_free = 0;
    for (int q = 0; q < n_sh + n_own; ++q) {
        const int r = q < n_sh ? q : own_lo + (q - n_sh);
        const int s0 = min(max(a.start[r], 0), a.n_verts), s1 = min(max(a.start[r + 1], 0), a.n_verts);
        const int n = min(s1 - s0, PO_RING_MAX_VERTS);
        const int flag = a.flags[r];
        if (n < 3 || (flag != PO_RING_SOLID && flag != PO_RING_FREE)) continue;  // (workgroup-uniform)
        const double *v = a.verts + 2 * (size_t)s0;  // s0 + n <= s1 <= n_verts: every read below stays inside verts
        unsigned par = 0;
        if (t == 0) s_count[0] = 0;
        __syncthreads();
        int round = 0;
        for (int e0 = 0; e0 < n; e0 += kThreads, ++round) {
            int *count = &s_count[round & 1];
            // ---- cull: one edge per thread ----
            if (t == 0) s_count[(round + 1) & 1] = 0;  // (the next round's counter: last read before the barrier that ended the previous round)
            const int e = e0 + t;
            if (e < n) {
                const int e1 = e + 1 == n ? 0 : e + 1;
                const double ax = v[2 * (size_t)e], ay = v[2 * (size_t)e + 1], bx = v[2 * (size_t)e1], by = v[2 * (size_t)e1 + 1];
                const bool above = ay > ymax && by > ymax, below = !(ay > ymin) && !(by > ymin), left = ax <= xmin && bx <= xmin;
                if (!(above || below || left)) {
                    const int slot = atomicAdd(count, 1);  // LDS; at most kThreads survivors per round, so slot < kThreads
                    s_edge[slot][0] = ax; s_edge[slot][1] = ay; s_edge[slot][2] = bx; s_edge[slot][3] = by;
                }
            }
            __syncthreads();
            // ---- test: four cell centres per thread against the survivors ----
            const int n_live = *count;
            for (int s = 0; s < n_live; ++s) {
                const double ax = s_edge[s][0], ay = s_edge[s][1], bx = s_edge[s][2], by = s_edge[s][3];
                if ((ay > py) != (by > py)) {
                    const bool up = by > ay;
                    const double ex = __dsub_rn(bx, ax), ey = __dsub_rn(by, ay);
                    const double ry = __dmul_rn(ex, __dsub_rn(py, ay));
#pragma unroll
                    for (int c = 0; c < kCells; ++c) {
                        const double cr = __dsub_rn(ry, __dmul_rn(ey, __dsub_rn(px[c], ax)));
                        if (up ? cr > 0.0 : cr < 0.0) par ^= 1u << c;
                    }
                }
            }
            __syncthreads();  // the LDS list is rewritten by the next round
        }
        if (flag == PO_RING_SOLID) occ |= par;
        else { has_free = true; in_free |= par; }
    }
    if (has_free) occ |= ~in_free & ((1u << kCells) - 1);

    if (j >= a.sy || i0 >= a.sx || occ == 0) return;
    unsigned char *dst = a.img + (size_t)k * (size_t)a.sx * (size_t)a.sy + (size_t)j * (size_t)a.sx + (size_t)i0;
    if (i0 + kCells <= a.sx) {
        uint32_t w, keep = 0xFFFFFFFFu;
        __builtin_memcpy(&w, dst, sizeof(w));  // (rows start at any byte address: an unaligned 4-byte access, which global memory serves)
#pragma unroll
        for (int c = 0; c < kCells; ++c)
            if (occ & (1u << c)) keep &= ~(0xFFu << (8 * c));
        if ((w & keep) != w) {
            w &= keep;
            __builtin_memcpy(dst, &w, sizeof(w));
        }
    } else {
        for (int c = 0; c < kCells && i0 + c < a.sx; ++c)
            if (occ & (1u << c)) dst[c] = 0;
    }
}

}  // namespace

// Every pointer inside *scene, pos_xy, world->cells and img are device pointers; img [M][sy][sx] holds po_launch_raster's image of scene->lists.  world == nullptr:
// the world clause is off.  The caller has checked what po_launch_raster asks for, n_rings >= 0, n_verts >= 0 and the world's sizes (1 <= wsx, wsy, wres > 0).
extern "C" hipError_t po_launch_scene(const po_scene *scene, int M, const double *pos_xy, const po_occupancy *world, int outside_occupied, unsigned char *img,
                                      hipStream_t st) {
    const po_rings &R = scene->rings;
    SceneArgs a{};
    a.verts = R.verts; a.start = R.start; a.flags = R.flags; a.first = R.first;
    a.n_rings = R.n_rings; a.n_verts = R.n_verts; a.n_shared = R.n_shared;
    if (world) {
        a.world = world->cells; a.wsx = world->size_x; a.wsy = world->size_y; a.outside = outside_occupied;
        a.wres = world->resolution; a.wpx = world->pos_x; a.wpy = world->pos_y;
    }
    a.sx = scene->lists.size_x; a.sy = scene->lists.size_y;
    a.res = scene->lists.resolution; a.px = scene->lists.pos_x; a.py = scene->lists.pos_y;
    a.pos_xy = pos_xy;
    a.img = img;
    const dim3 grid((a.sx + kTileX - 1) / kTileX, (a.sy + kTileY - 1) / kTileY, M);
    hipLaunchKernelGGL(scene_overlay_kernel, grid, dim3(kThreads), 0, st, a);
    return hipGetLastError();
}
