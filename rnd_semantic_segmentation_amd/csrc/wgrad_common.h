// What the weight-gradient kernels of igemm_tn.hip (wgrad_tn / s4 / tn256 / q3 / p3) and gconv.hip (gwgrad / gwgrad3 and their table-driven twins) share:
// the workgroup decode, the accumulator -> slab epilogue, the pixel-coordinate advance and the split cost model.  The main loops stay in the kernels
// (depths, vmcnt counts and staging differ on purpose); these are the pieces around them that must stay identical by construction.
#pragma once
#include "mi_common.h"

// ---- workgroup decode: block id -> (output tile, middle index, K split) -> tile origin and the split's pixel range ---------------------------------
// The workgroups of one (split, middle index) - which all stream the same pixel rows - are consecutive logical ids; mi_xcd_remap puts consecutive logical
// ids on one XCD, so those rows are fetched into one L2 instead of eight.  `mid` counts whatever the launch has between tile and split: the tap
// (nmid = T: wgrad_tn, wgrad_tn256, gwgrad), the kernel row (nmid = 3 or kh: q3, p3, gwgrad3) or nothing (nmid = 1: s4).
struct WgDecode {
    int tile, mid, split;      // tile = ot * i_tiles + it
    int o0, i0;                // first output / input channel of the tile
    int m_begin, m_end, nk;    // the split's pixel rows [m_begin, m_end) and its K steps (<= 0: nothing to do)
};
// COND_REMAP: the remap is a launch parameter (gconv: MI_GCONV_REMAP), otherwise unconditional
template <int TO_, int TI_, bool COND_REMAP = false>
__device__ __forceinline__ WgDecode wg_decode_tile(int bid, int nblk, int o_tiles, int i_tiles, int nmid, int remap = 1) {
    WgDecode w;
    const int tiles = o_tiles * i_tiles;
    const int logical = (!COND_REMAP || remap) ? mi_xcd_remap(bid, nblk) : bid;
    w.tile = logical % tiles;
    const int rest = logical / tiles;
    w.mid = rest % nmid;
    w.split = rest / nmid;
    const int ot = w.tile / i_tiles, it = w.tile - ot * i_tiles;
    w.o0 = ot * TO_;
    w.i0 = it * TI_;
    w.m_begin = w.m_end = w.nk = 0;
    return w;
}
// ... and the pixel range of the split in K steps of KP_ pixels (the fused-row kernels of igemm_tn.hip count padded coordinates instead: wg_decode_tile)
template <int TO_, int TI_, int KP_, bool COND_REMAP = false>
__device__ __forceinline__ WgDecode wg_decode(int bid, int nblk, int o_tiles, int i_tiles, int nmid, int M, int rows_per_split, int remap = 1) {
    WgDecode w = wg_decode_tile<TO_, TI_, COND_REMAP>(bid, nblk, o_tiles, i_tiles, nmid, remap);
    w.m_begin = w.split * rows_per_split;
    w.m_end = min(M, w.m_begin + rows_per_split);
    w.nk = (w.m_end - w.m_begin + KP_ - 1) / KP_;
    return w;
}

// ---- accumulator -> slab: the 16x16 MFMA D fragments acc[a][b] of a wave, D rows = i, D columns = o ------------------------------------------------
// slab[o][i], i fastest, row_stride floats per o; the lane owns o = o_base + 16 b + (lane & 15) and the four consecutive i from i_base + 16 a + 4 (lane >> 4),
// bounded by O and i_bound (igemm_tn: row_stride = i_bound = I, a multiple of 8; gconv: both roundup(I, 4)).
// write_through: sc1 stores (mi_st2_sc1) - the slab is handed to another workgroup of the SAME launch, possibly on another XCD (gwgrad_body's ticket path).
template <int NA, int NB>
__device__ __forceinline__ void slab_store(float* slab, int row_stride, int O, int i_bound, int o_base, int i_base, int lane, const f32x4 (&acc)[NA][NB],
                                           bool write_through = false) {
    const int fcol = lane & 15, fq = lane >> 4;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int o = o_base + b * 16 + fcol;
        if (o >= O) continue;
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            const int i = i_base + a * 16 + fq * 4;
            if (i >= i_bound) continue;
            float* dst = slab + (long)o * row_stride + i;
            if (write_through) {
                mi_st2_sc1(dst, acc[a][b][0], acc[a][b][1]);
                mi_st2_sc1(dst + 2, acc[a][b][2], acc[a][b][3]);
            } else {
                *reinterpret_cast<f32x4*>(dst) = acc[a][b];
            }
        }
    }
}

// ---- pixel coordinate (row h, column w) of an H x W map advanced by a fixed step of step_rows < H rows + step_cols < W columns: selects only, every
// coordinate wraps at most once, so a main loop that calls this stays one basic block.  Returns 1 when the row wrapped into the next image.
__device__ __forceinline__ int px_advance(int& h, int& w, int step_rows, int step_cols, int H, int W) {
    const int w1 = w + step_cols;
    const bool cw = w1 >= W;
    w = cw ? w1 - W : w1;
    const int h1 = h + step_rows + (cw ? 1 : 0);
    const bool ch = h1 >= H;
    h = ch ? h1 - H : h1;
    return ch ? 1 : 0;
}

// ---- K splits of a launch of `tiles` workgroups per split over M pixels (host) ----------------------------------------------------------------------
// Minimise rounds x (K steps per split + fixed_steps), where a round is `slots` resident workgroups and fixed_steps is a workgroup's prologue, pipeline
// fill and slab write in units of a K step of step_px pixels; never fewer than min_steps K steps per split, at most max_s splits.
inline int wgrad_pick_splits(long M, int tiles, int step_px, int min_steps, int fixed_steps, int slots, int max_s) {
    const long steps = (M + step_px - 1) / step_px;
    int best = 1;
    double best_cost = 1e30;
    for (int s = 1; s <= max_s; ++s) {
        const long per = (steps + s - 1) / s;
        if (s > 1 && per < min_steps) break;
        const long rounds = ((long)tiles * s + slots - 1) / slots;
        const double cost = (double)rounds * (double)(per + fixed_steps);
        if (cost < best_cost - 1e-9) {
            best_cost = cost;
            best = s;
        }
    }
    return best;
}
