// po_edt.hip — exact Euclidean distance transform of an occupancy image on the device (gfx950): the obstacle-distance layer every map stage reads,
// built from what a planner has in its hands.  Replaces the host lines of the reference's callers (src/test/path_optimizer_benchmark.cpp:38-43, demo.cpp:108)
//     cv::distanceTransform(binary, distance, CV_DIST_L2, CV_DIST_MASK_PRECISE);  distance *= resolution;
//
// Definition (include/po_hip.h):
//     d2(i, j)   = min over occupied (p, q) of (i - p)^2 + (j - q)^2                    exact, int32
//     dist(i, j) = float32(sqrt(double(d2))) * float32(resolution)                        one float32 multiply (this object is compiled with -ffp-contract=off)
//     no occupied cell in the image: every cell = float32(sqrt(double(size_x^2 + size_y^2))) * float32(resolution)   (the project's own rule)
// Layout: [M][size_y][size_x], x contiguous, for the image (unsigned char, 0 = occupied) and the layer (float) alike.
//
// Separable, two launches on one stream, integers only until the final square root:
//   edt_columns_kernel  along y.  One workgroup = a strip of 32 columns (lane = column: every load / store of a half-wave is one contiguous row piece) x 32 segments
//       of the column (threadIdx.y).  Phase 1: every thread walks its segment upwards, writes the distance to the next occupied cell BELOW-or-at inside the segment
//       (0xFFFF: none) and leaves the segment's first / last occupied row in LDS.  Phase 2 (after one barrier): the carries — the nearest occupied row before the
//       segment and after it — come from at most 31 LDS words each; the thread walks downwards and writes g = min(distance up, distance down), 0xFFFF when the
//       whole column is free.  Rows travel in batches of 16 (loads, scan in registers, stores), so a thread waits for memory once per batch and not once per row.
//       No thread walks a whole column: a 495 x 497 image is 16 workgroups x 1024 lanes with 16 rows each.
//   edt_rows_kernel     along x.  One workgroup = one row: g^2 of the row in LDS (int32, 4 bytes per cell, 16 KB at 4096), then per cell the bounded search
//       best = min(g(x)^2, min over d >= 1 with d^2 < best of d^2 + g(x -+ d)^2): only offsets that can still improve are read, so the work per cell is
//       proportional to its distance (four offsets per trip: independent LDS reads).  The layer is written once, coalesced (lane = x).
// Sentinel: kFar = 0x3FFFFFFF stands for "no occupied cell in this column"; the largest squared offset added to it is 4098^2 (the search reads up to three offsets past the row), the sum stays below 2^31; the largest
// real d2 is 2 * 4095^2 < kFar.  A row whose g are ALL kFar means an image without any occupied cell (g is a property of the column), which is how the no-obstacle
// rule is detected without a pass of its own.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "po_launch.hpp"

namespace {

constexpr int kMaxSide = 4096;      // LDS row of edt_rows_kernel, range of the 16-bit intermediate and of the int32 sentinel arithmetic
constexpr int kStrip = 32;          // columns per workgroup of edt_columns_kernel
constexpr int kSegs = 32;           // segments per column
constexpr int kBatch = 16;          // rows a thread of edt_columns_kernel has in flight: loads first, then the scan in registers, then the stores
constexpr int kRowThreads = 256;
constexpr int kStep = 4;            // offsets per trip of the bounded search (independent LDS reads; the bound is tested once per trip)
constexpr int kFar = 0x3FFFFFFF;
constexpr unsigned short kNone = 0xFFFF;

__global__ __launch_bounds__(kStrip *kSegs) void edt_columns_kernel(const unsigned char *__restrict__ cells, unsigned short *__restrict__ g, int sx, int sy) {
    __shared__ int first_row[kSegs][kStrip], last_row[kSegs][kStrip];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int x = blockIdx.x * kStrip + tx;
    const bool live = x < sx;
    const size_t img = (size_t)blockIdx.y * (size_t)sx * (size_t)sy;
    const int seg = (sy + kSegs - 1) / kSegs;
    const int r0 = min(ty * seg, sy), r1 = min(r0 + seg, sy);
    const unsigned char *c = cells + img + x;
    unsigned short *gc = g + img + x;

    // phase 1: upwards; distance to the next occupied row at or below, inside the segment
    int first = -1, last = -1;
    if (live) {
        int next = -1;
        for (int yb = r1; yb > r0; yb -= kBatch) {
            int v[kBatch];  // (a register each, and addresses clamped into the segment instead of predicated loads: the 16 loads are issued back to back)
#pragma unroll
            for (int k = 0; k < kBatch; ++k) v[k] = c[(size_t)max(yb - 1 - k, r0) * sx];
#pragma unroll
            for (int k = 0; k < kBatch; ++k) {
                const int y = yb - 1 - k;
                if (y >= r0) {
                    if (v[k] == 0) {
                        next = y;
                        first = y;
                        if (last < 0) last = y;
                    }
                    gc[(size_t)y * sx] = next < 0 ? kNone : (unsigned short)(next - y);
                }
            }
        }
    }
    first_row[ty][tx] = first;
    last_row[ty][tx] = last;
    __syncthreads();
    if (!live) return;

    // carries: nearest occupied row above the segment, nearest below it
    int up = -1, down = -1;
    for (int t = ty - 1; t >= 0; --t)
        if (last_row[t][tx] >= 0) { up = last_row[t][tx]; break; }
    for (int t = ty + 1; t < kSegs; ++t)
        if (first_row[t][tx] >= 0) { down = first_row[t][tx]; break; }

    // phase 2: downwards; what phase 1 wrote tells where the occupied cells are (0) and how far the next one inside the segment is
    for (int yb = r0; yb < r1; yb += kBatch) {
        int v[kBatch];
#pragma unroll
        for (int k = 0; k < kBatch; ++k) v[k] = gc[(size_t)min(yb + k, r1 - 1) * sx];
#pragma unroll
        for (int k = 0; k < kBatch; ++k) {
            const int y = yb + k;
            if (y < r1) {
                if (v[k] == 0) up = y;
                int d = v[k] != kNone ? (int)v[k] : (down >= 0 ? down - y : (int)kNone);
                if (up >= 0) d = min(d, y - up);
                gc[(size_t)y * sx] = (unsigned short)d;
            }
        }
    }
}

__global__ __launch_bounds__(kRowThreads) void edt_rows_kernel(const unsigned short *__restrict__ g, float *__restrict__ out, int sx, int sy, float res) {
    __shared__ int gsq[kMaxSide + 2];  // g^2 of the row at [1 .. sx]; [0] and [sx + 1] = kFar stand for everything outside the row
    const size_t row = ((size_t)blockIdx.y * (size_t)sy + blockIdx.x) * (size_t)sx;
    int any = 0;
    for (int x = threadIdx.x; x < sx; x += kRowThreads) {
        const int v = g[row + x];
        gsq[x + 1] = v == kNone ? kFar : v * v;
        any |= v != kNone;
    }
    if (threadIdx.x == 0) gsq[0] = gsq[sx + 1] = kFar;
    any = __syncthreads_or(any);
    if (!any) {  // the image has no occupied cell: the project's rule
        const float far = (float)sqrt((double)(sx * sx + sy * sy)) * res;
        for (int x = threadIdx.x; x < sx; x += kRowThreads) out[row + x] = far;
        return;
    }
    for (int x = threadIdx.x; x < sx; x += kRowThreads) {
        int best = gsq[x + 1];
        // every candidate d^2 + g(x -+ d)^2 is the squared distance to some occupied cell, so reading a few offsets past the bound changes nothing
        for (int d = 1; d < sx && d * d < best; d += kStep) {
#pragma unroll
            for (int k = 0; k < kStep; ++k) {
                const int e = d + k;  // (e <= 4098: e * e + kFar < 2^31)
                best = min(best, e * e + min(gsq[max(x - e, -1) + 1], gsq[min(x + e, sx) + 1]));
            }
        }
        // float32(sqrt(double(n))) is the correctly rounded float32 root of the integer n (53 >= 2 * 24 + 2 bits)
        out[row + x] = (float)sqrt((double)best) * res;
    }
}

}  // namespace

extern "C" int po_edt_max_side(void) { return kMaxSide; }
extern "C" int po_edt_max_images(void) { return 65535; }  // grid.y
// bytes of the 16-bit intermediate (g, one value per cell)
extern "C" size_t po_edt_scratch_bytes(int M, int sx, int sy) { return sizeof(unsigned short) * (size_t)M * (size_t)sx * (size_t)sy; }

// cells [M][sy][sx] -> out [M][sy][sx]; scratch: po_edt_scratch_bytes.  The caller has checked 1 <= sx, sy <= po_edt_max_side(), 1 <= M <= po_edt_max_images().
extern "C" hipError_t po_launch_edt(const unsigned char *cells, int M, int sx, int sy, float res, void *scratch, float *out, hipStream_t st) {
    unsigned short *g = static_cast<unsigned short *>(scratch);
    hipLaunchKernelGGL(edt_columns_kernel, dim3((sx + kStrip - 1) / kStrip, M), dim3(kStrip, kSegs), 0, st, cells, g, sx, sy);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(edt_rows_kernel, dim3(sy, M), dim3(kRowThreads), 0, st, g, out, sx, sy, res);
    return hipGetLastError();
}
