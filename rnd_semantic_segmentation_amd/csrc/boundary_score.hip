// Boundary IoU and trimap IoU of one picture (mi_boundary_score, TEST.BOUNDARY): from the predicted mask and the label, for both class maps
//   G = the label where it lies in [0, K), else 255;   P = 255 where the label is ignore_index, else the prediction (>= K counts as 255)
// the number of 3 x 3 erosions e_L(p) <= D that every pixel survives in the binary mask of its own class, and five histograms over (class, e)
// from which host/metrics.py (boundary_summary) reads both metrics at every band width d <= D.  The definition: include/mi355seg.h.
// Integers only - no floating point, integer atomics - so two calls give the same bits.  Two launches, nothing read back in between.
//   rows      one wave walks a segment of a row in chunks of 64 pixels.  A chunk's run starts are one ballot per map; with the masks of the
//             chunk before and the chunk after, a lane reads its distance to the run's two ends (capped at D <= 64) from two bit scans.
//             Writes G, P and the two half-widths a_G, a_P as one 32-bit word per pixel into the workspace.
//   columns   one lane per pixel, a wave on 64 neighbouring pixels of a row.  The lane walks r = 1, 2, ... over the rows y - r and y + r of its
//             column, keeping the running minimum of a, for both maps at once (one word per row visited), until both walks have ended.  The five
//             cells go into the workgroup's LDS table of 32-bit counters, aggregated in the wave first (an interior is one cell for 64 lanes), and
//             the table is flushed with one 64-bit atomic per non-zero cell.
#include "mi_common.h"

namespace {

constexpr int BS_MAX_K = 32;
constexpr int BS_MAX_D = 64;
constexpr int BS_MAPS = 5;           // the histograms of include/mi355seg.h
constexpr int BS_SEG = 8;            // chunks of 64 pixels a wave of the row pass walks (plus one chunk of context on either side)
constexpr int BS_WG_TARGET = 4096;   // workgroups the column pass aims for: smaller tiles were faster at 1024 x 2048 ...
constexpr int BS_MIN_ROWS = 8;       // ... but each zeroes and flushes a table of up to 10 400 cells: at least two rows per wave (the one-off
                                     // experiment behind both values: DESIGN.md 4.4h)
constexpr int BS_MAX_ROWS = 64;      // rows of a tile of the column pass at most (four waves, a row each, in turn)
constexpr long BS_MAX_GRID = 1l << 16;      // workgroups of either launch at most: beyond it a workgroup strides over the row segments / the tiles, so that
                                     // no shape the entry accepts (H * W < 2^31: up to 5 * 10^8 row segments) asks for a grid the runtime may reject
constexpr int BS_PEEL = 2;           // in-wave aggregation rounds per cell: interiors are one cell per wave, a band next to an interior two
constexpr unsigned BS_NONE = 255u;

typedef unsigned long long u64;

struct BsPlan {
    int chunks, segs;                // row pass: chunks per row, wave segments per row
    long row_waves;                  // H * segs
    int tiles_x, rows, row_groups;   // column pass: 64-column tiles, rows per workgroup
};
inline BsPlan bs_plan(int H, int W) {
    BsPlan p;
    p.chunks = (W + 63) / 64;
    p.segs = (p.chunks + BS_SEG - 1) / BS_SEG;
    p.row_waves = (long)H * p.segs;
    p.tiles_x = p.chunks;
    const long units = (long)H * p.tiles_x;
    long rows = (units + BS_WG_TARGET - 1) / BS_WG_TARGET;
    rows = (rows + 3) & ~3l;         // the four waves take the same number of rows
    p.rows = (int)(rows < BS_MIN_ROWS ? BS_MIN_ROWS : (rows > BS_MAX_ROWS ? BS_MAX_ROWS : rows));
    p.row_groups = (H + p.rows - 1) / p.rows;
    return p;
}

// G | P << 8 of pixel `idx`
__device__ __forceinline__ unsigned bs_classes(const uint8_t* __restrict__ pred, const long long* __restrict__ lab, long idx, int K, int ignore_index) {
    const long long l = lab[idx];
    const unsigned pr = pred[idx];
    const unsigned g = (l >= 0 && l < K) ? (unsigned)l : BS_NONE;
    const unsigned p = (l == ignore_index || pr >= (unsigned)K) ? BS_NONE : pr;
    return g | (p << 8);
}

// One chunk of a row: v = G | P << 8 of the lane's pixel (both 255 beyond the row), bg / bp = the lanes where a run of G / P starts.  Column 0
// starts a run, and so does column W, one past the row: the picture's edge ends every run.  A chunk outside [0, W] has no starts.
struct BsChunk {
    unsigned v;
    u64 bg, bp;
};
__device__ __forceinline__ BsChunk bs_chunk(const uint8_t* __restrict__ pred, const long long* __restrict__ lab, long row0, int c, int W, int K,
                                            int ignore_index, int lane) {
    BsChunk ch;
    ch.v = BS_NONE | (BS_NONE << 8);
    ch.bg = ch.bp = 0ull;
    if (c < 0 || (long)c * 64 > W) return ch;          // wave-uniform
    const int x = c * 64 + lane;
    if (x < W) ch.v = bs_classes(pred, lab, row0 + x, K, ignore_index);
    unsigned before = (unsigned)__shfl_up((int)ch.v, 1);
    if (lane == 0 && x > 0 && x <= W) before = bs_classes(pred, lab, row0 + x - 1, K, ignore_index);
    const bool edge = x == 0 || x == W;
    const bool inside = x > 0 && x < W;
    ch.bg = __ballot(edge || (inside && (ch.v & 255u) != (before & 255u)));
    ch.bp = __ballot(edge || (inside && (ch.v >> 8) != (before >> 8)));
    return ch;
}

// min(D, the largest r with columns x - r .. x + r inside the run of the lane's pixel) from the run starts of three neighbouring chunks
__device__ __forceinline__ unsigned bs_half_width(u64 prev, u64 cur, u64 next, int lane, int D) {
    const u64 upto = cur & (~0ull >> (63 - lane));                     // starts at lanes <= mine: the run's own start is the highest
    int left = BS_MAX_D, right = BS_MAX_D;
    if (upto) left = lane - (63 - __clzll((long long)upto));
    else if (prev) left = lane + 1 + __clzll((long long)prev);
    const u64 after = lane == 63 ? 0ull : cur & (~0ull << (lane + 1));  // starts at lanes > mine: the lowest is one past the run's end
    if (after) right = __ffsll((long long)after) - 2 - lane;
    else if (next) right = 62 + __ffsll((long long)next) - lane;
    return (unsigned)min(D, min(left, right));
}

__global__ __launch_bounds__(256) void boundary_rows_kernel(const uint8_t* __restrict__ pred, const long long* __restrict__ lab, int H, int W, int K,
                                                            int ignore_index, int D, int chunks, int segs, long row_waves,
                                                            unsigned* __restrict__ ws) {
    const int lane = threadIdx.x & 63;
    for (long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6); wave < row_waves; wave += (long)gridDim.x * 4) {      // wave-uniform
        const int y = (int)(wave / segs), seg = (int)(wave % segs);
        const long row0 = (long)y * W;
        const int c_lo = seg * BS_SEG, c_hi = min(chunks, c_lo + BS_SEG);
        BsChunk prev = bs_chunk(pred, lab, row0, c_lo - 1, W, K, ignore_index, lane);
        BsChunk cur = bs_chunk(pred, lab, row0, c_lo, W, K, ignore_index, lane);
        for (int c = c_lo; c < c_hi; ++c) {
            const BsChunk next = bs_chunk(pred, lab, row0, c + 1, W, K, ignore_index, lane);
            const int x = c * 64 + lane;
            if (x < W) {
                const unsigned ag = bs_half_width(prev.bg, cur.bg, next.bg, lane, D);
                const unsigned ap = bs_half_width(prev.bp, cur.bp, next.bp, lane, D);
                ws[row0 + x] = cur.v | (ag << 16) | (ap << 24);
            }
            prev = cur;
            cur = next;
        }
    }
}

// One cell of the workgroup's table.  BS_PEEL rounds of in-wave aggregation (the peel of polyp_score.hip): the lanes that hold the cell of the
// first lane still waiting retire, their leader adds their number; what is left adds one by one.  Every lane of the wave calls.
__device__ __forceinline__ void bs_hist_add(unsigned* tab, unsigned key, bool live, int lane) {
    unsigned add = live ? 1u : 0u;
    bool waiting = live;
#pragma unroll
    for (int r = 0; r < BS_PEEL; ++r) {
        if (waiting) {
            const unsigned k0 = (unsigned)__builtin_amdgcn_readfirstlane((int)key);
            const bool same = key == k0;
            const u64 m = __ballot(same);              // among the lanes still waiting
            if (same) {
                waiting = false;
                add = lane == __ffsll((long long)m) - 1 ? (unsigned)__popcll(m) : 0u;
            }
        }
    }
    if (add) atomicAdd(&tab[key], add);
}

__global__ __launch_bounds__(256) void boundary_cols_kernel(const unsigned* __restrict__ ws, int H, int W, int K, int D, int rows, int tiles_x,
                                                            long tiles, u64* __restrict__ hist) {
    extern __shared__ unsigned bs_tab[];               // [5][K][D + 1]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int D1 = D + 1, cells = BS_MAPS * K * D1;
    for (int c = tid; c < cells; c += 256) bs_tab[c] = 0u;
    __syncthreads();
    for (long t = blockIdx.x; t < tiles; t += gridDim.x) {             // one tile per workgroup unless the grid is capped (BS_MAX_GRID)
        const int tile = (int)(t % tiles_x), rg = (int)(t / tiles_x);
        const int x = tile * 64 + lane;
        const int ya = rg * rows, yb = min(H, ya + rows);
        const bool in_x = x < W;
        for (int y = ya + wave; y < yb; y += 4) {          // wave-uniform bounds
            unsigned g = BS_NONE, p = BS_NONE;
            int eg = 0, ep = 0;
            if (in_x) {
                const unsigned w0 = ws[(long)y * W + x];
                g = w0 & 255u;
                p = (w0 >> 8) & 255u;
                int mg = (int)((w0 >> 16) & 255u), mp = (int)(w0 >> 24);
                bool walk_g = g != BS_NONE, walk_p = p != BS_NONE;
                const int reach = min(D, min(y, H - 1 - y));                 // rows y - r and y + r exist
                for (int r = 1; r <= reach && (walk_g || walk_p); ++r) {
                    const unsigned up = ws[(long)(y - r) * W + x], dn = ws[(long)(y + r) * W + x];
                    if (walk_g) {
                        mg = min(mg, (int)min((up >> 16) & 255u, (dn >> 16) & 255u));
                        if ((up & 255u) == g && (dn & 255u) == g && mg >= r) eg = r;
                        else walk_g = false;
                    }
                    if (walk_p) {
                        mp = min(mp, (int)min(up >> 24, dn >> 24));
                        if (((up >> 8) & 255u) == p && ((dn >> 8) & 255u) == p && mp >= r) ep = r;
                        else walk_p = false;
                    }
                }
            }
            const bool has_g = g != BS_NONE, has_p = p != BS_NONE, hit = has_g && g == p;
            const unsigned kg = has_g ? g : 0u, kp = has_p ? p : 0u;        // a lane that is not live still forms a key inside the table
            bs_hist_add(bs_tab, (0u * K + kg) * D1 + eg, has_g, lane);
            bs_hist_add(bs_tab, (1u * K + kp) * D1 + ep, has_p, lane);
            bs_hist_add(bs_tab, (2u * K + kg) * D1 + max(eg, ep), hit, lane);
            bs_hist_add(bs_tab, (3u * K + kg) * D1 + eg, hit, lane);
            bs_hist_add(bs_tab, (4u * K + kp) * D1 + eg, has_p && has_g, lane);
        }
    }
    __syncthreads();
    for (int c = tid; c < cells; c += 256) {
        const unsigned v = bs_tab[c];
        if (v) atomicAdd(&hist[c], (u64)v);
    }
}

}  // namespace

extern "C" size_t mi_boundary_score_workspace(int H, int W) {
    if (H <= 0 || W <= 0 || (long)H * W >= (1l << 31)) return 0;
    return ((size_t)H * (size_t)W * sizeof(unsigned) + 255) & ~(size_t)255;
}

extern "C" int mi_boundary_score(const uint8_t* pred, const int64_t* labels, int H, int W, int K, int ignore_index, int D, int64_t* hist, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    MI_REQUIRE(pred && labels && hist, "mi_boundary_score: null operand");
    MI_REQUIRE(workspace, "mi_boundary_score: null workspace");
    MI_REQUIRE(H > 0 && W > 0, "mi_boundary_score: bad dimension (picture %d x %d)", H, W);
    MI_REQUIRE((long)H * W < (1l << 31), "mi_boundary_score: H * W = %ld reaches 2^31", (long)H * W);
    MI_REQUIRE(K >= 1 && K <= BS_MAX_K, "mi_boundary_score: K %d lies outside 1..%d", K, BS_MAX_K);
    MI_REQUIRE(D >= 1 && D <= BS_MAX_D, "mi_boundary_score: D %d lies outside 1..%d", D, BS_MAX_D);
    MI_REQUIRE(ignore_index < 0 || ignore_index >= K, "mi_boundary_score: ignore_index %d names a class (K %d)", ignore_index, K);
    MI_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3) == 0, "mi_boundary_score: workspace must be 4-byte aligned");
    const size_t need = mi_boundary_score_workspace(H, W);
    if (workspace_bytes < need) return mi_set_error(MI_ENOMEM, "mi_boundary_score: workspace too small (%zu < %zu bytes)", workspace_bytes, need);
    const BsPlan p = bs_plan(H, W);
    unsigned* ws = reinterpret_cast<unsigned*>(workspace);
    const long long* lab = reinterpret_cast<const long long*>(labels);
    hipStream_t s = (hipStream_t)stream;
    const long row_wgs = (p.row_waves + 3) / 4, tiles = (long)p.row_groups * p.tiles_x;
    hipLaunchKernelGGL(boundary_rows_kernel, dim3((unsigned)(row_wgs < BS_MAX_GRID ? row_wgs : BS_MAX_GRID)), dim3(256), 0, s, pred, lab, H, W, K,
                       ignore_index, D, p.chunks, p.segs, p.row_waves, ws);
    MI_CHECK_LAUNCH("mi_boundary_score (row pass)");             // a rejected row pass must not be followed by a column pass over an unwritten workspace
    const size_t lds = (size_t)BS_MAPS * K * (D + 1) * sizeof(unsigned);
    hipLaunchKernelGGL(boundary_cols_kernel, dim3((unsigned)(tiles < BS_MAX_GRID ? tiles : BS_MAX_GRID)), dim3(256), lds, s, ws, H, W, K, D, p.rows,
                       p.tiles_x, tiles, reinterpret_cast<u64*>(hist));
    MI_CHECK_LAUNCH("mi_boundary_score");
    return MI_OK;
}
