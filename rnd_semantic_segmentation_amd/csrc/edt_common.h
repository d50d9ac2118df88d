// The two passes of the exact Euclidean distance transform that surface_score.hip (distances between two surfaces) and signed_distance.hip (the signed
// distance map of a mask) share.  Two site maps travel together: a 32-bit word per pixel holds g of map 0 in its low half and g of map 1 in its high
// half, g(x, y) = the vertical distance to the nearest site of the column (EDT_NONE: the column has none; never squared).
//   edt_sweep_column   one lane per column: a down sweep and an up sweep over the column write g of both maps
//   edt_query          d2 = min over x' of (x - x')^2 + g(x', y)^2 for one pixel, the row of g in LDS, scanning x' outward from x
// Integers only: d2 is exact and two calls give the same bits.
#pragma once
#include "mi_common.h"

constexpr int EDT_MAX_SIDE = 4096;           // d2 <= 2 * 4095^2 < 2^25; a row of g fits in 16 KiB of LDS
constexpr int EDT_D2_BITS = 25;
constexpr unsigned EDT_D2_MASK = (1u << EDT_D2_BITS) - 1u;
constexpr unsigned EDT_NONE = 0xffffu;       // g of a column without a site

// g(x, y) of both maps for one column: `sites(y)` returns bit 0 = the pixel is a site of map 0, bit 1 = of map 1; `o` points at the column's first
// word, rows W words apart.  Eight rows are loaded before any is used, the carried state (the last site seen) is two registers.
template <class Sites>
__device__ __forceinline__ void edt_sweep_column(Sites sites, unsigned* __restrict__ o, int H, int W) {
    int last_p = -1, last_g = -1;
    for (int y0 = 0; y0 < H; y0 += 8) {                            // down: the nearest site at or above y
        unsigned v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = y0 + k < H ? sites(y0 + k) : 0u;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int y = y0 + k;
            if (y < H) {
                if (v[k] & 1u) last_p = y;
                if (v[k] & 2u) last_g = y;
                const unsigned dp = last_p < 0 ? EDT_NONE : (unsigned)(y - last_p), dg = last_g < 0 ? EDT_NONE : (unsigned)(y - last_g);
                o[(long)y * W] = dp | (dg << 16);
            }
        }
    }
    int next_p = -1, next_g = -1;
    for (int y1 = H - 1; y1 >= 0; y1 -= 8) {                       // up: the nearest site at or below y; reads what this thread wrote
        unsigned v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = y1 - k >= 0 ? o[(long)(y1 - k) * W] : 0xffffffffu;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int y = y1 - k;
            if (y >= 0) {
                unsigned dp = v[k] & 0xffffu, dg = v[k] >> 16;
                if (dp == 0u) next_p = y;
                if (dg == 0u) next_g = y;
                if (next_p >= 0) dp = min(dp, (unsigned)(next_p - y));
                if (next_g >= 0) dg = min(dg, (unsigned)(next_g - y));
                o[(long)y * W] = dp | (dg << 16);
            }
        }
    }
}

// d2 of the pixel at column x to the sites of the map whose g sits at `shift` in the row's words.  The sentinel is never squared.  The scan stops
// at the first dx with dx^2 >= best: every column from there on offers at least dx^2, so it cannot lower the minimum (a tie leaves it as it is).
// The caller queries only where the map has a site somewhere in the image: best is finite; the mask keeps an index in bounds regardless.
__device__ __forceinline__ unsigned edt_query(const unsigned* row, int x, int W, int shift) {
    unsigned gv = (row[x] >> shift) & 0xffffu;
    unsigned best = gv == EDT_NONE ? 0xffffffffu : gv * gv;
    const int reach = max(x, W - 1 - x);
    for (int dx = 1; dx <= reach; ++dx) {
        const unsigned dx2 = (unsigned)(dx * dx);
        if (dx2 >= best) break;
        if (x - dx >= 0) {
            gv = (row[x - dx] >> shift) & 0xffffu;
            if (gv != EDT_NONE) best = min(best, dx2 + gv * gv);
        }
        if (x + dx < W) {
            gv = (row[x + dx] >> shift) & 0xffffu;
            if (gv != EDT_NONE) best = min(best, dx2 + gv * gv);
        }
    }
    return best & EDT_D2_MASK;
}
