// The 7x7 / stride 2 / pad 3 stem conv (resnet.py:137) on raw image rows: no patch matrix in forward or backward.
//
// The image is packed once as bf16 [B][H][W][4] (channel 3 = 0): 8 bytes per pixel.  A workgroup stages the raw image rows of its tile into LDS
// (out-of-image halo zero-filled there), so the windows of neighbouring output pixels, which overlap, are read from HBM once per tile.
//   forward          y[b][ho][wo][o] = sum_k x[b][2ho-3+ky][2wo-3+kx][c] * w[o][k], k = (c*7 + ky)*7 + kx, gathered from the staged rows and contracted
//                    in the order of the patch-matrix GEMM this replaces: y has that route's bits (raw conv output, rounded to bf16)
//   weight gradient  dw[o][ky][k]    = sum_(b,ho,wo) dy[b][ho][wo][o] * x4[b][2ho-3+ky][(2wo-3)*4 + k], k = kx*4 + c: for one kernel row the 7 input
//                    pixels of output pixel wo are 28 contiguous bf16 at pixel column 2wo - 3, padded to 32.  The contraction runs over pixels and
//                    both operands are read from LDS with ds_read_b64_tr_b16, as in igemm_tn.hip; the x operand is the staged image row itself,
//                    read as overlapping 64-byte "patch rows" 16 bytes apart.  Elements k = 28..31 belong to pixel column 2wo + 4, outside the
//                    window, and c = 3 is the zero channel: the reducer drops both.
#include "mi_common.h"

namespace {

constexpr int SD_TW = 64;                    // output columns of a tile: 4 groups of 16 (one MFMA column / row group each)
constexpr int SD_ROWPX = 136;                // staged pixels per image row: 2*64 + 5 window pixels, 1 for k = 28..31 of the last window, 2 pad
constexpr int SD_ROWB = SD_ROWPX * 8;        // 1088 bytes, a multiple of 16: pixel column 2*wo0 - 3 sits at byte 0 of every staged row
constexpr int SD_FWD_TH = 8;                 // output rows of a forward tile
constexpr int SD_FWD_ROWS = 2 * SD_FWD_TH + 5;
constexpr int SD_KB = 6;                     // K steps of the forward: the 147 window elements in OIHW order, padded to 192 like the patch matrix was
constexpr int SD_WG_TH = 4;                  // output rows of a weight-gradient tile
constexpr int SD_WG_ROWS = 2 * SD_WG_TH + 5;
constexpr int SD_DYROWB = SD_TW * 128;       // one staged dy row: 64 pixels x 64 channels bf16
constexpr int SD_PART = 64 * 7 * 32;         // floats of one weight-gradient partial [o][ky][k]
constexpr int SD_PP_ROWS = SD_WG_TH / 2 + 1; // pooled rows whose 3x3/2/1 windows reach a weight-gradient tile's 4 conv rows (the tile starts on an even row)
constexpr int SD_PP_COLS = SD_TW / 2 + 1;    // ... and pooled columns that reach its 64 conv columns
constexpr int SD_PP_ITEMS = SD_PP_ROWS * SD_PP_COLS * 8;      // (pooled pixel, 8-channel chunk) items of that patch

// ---- image pack -----------------------------------------------------------------------------------------------------------------------------
// fp32 NCHW -> bf16 [B][H][W][4]: a thread converts pixels p, p + 256, p + 512, p + 768 of its block's 1024 (every load instruction of a wave
// is 256 contiguous bytes of one plane, every store 512 contiguous bytes)
__global__ __launch_bounds__(256) void stem_pack_f32_kernel(const float* __restrict__ x, bf16x4* __restrict__ x4, long HW, int B) {
    const int b = blockIdx.y;
    const float* img = x + (long)b * 3 * HW;
    const long p0 = (long)blockIdx.x * 1024 + threadIdx.x;
    float v[4][3];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long p = p0 + j * 256;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[j][c] = p < HW ? img[c * HW + p] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long p = p0 + j * 256;
        if (p < HW) {
            bf16x4 o;
            o[0] = (__bf16)v[j][0];
            o[1] = (__bf16)v[j][1];
            o[2] = (__bf16)v[j][2];
            o[3] = (__bf16)0.f;
            x4[(long)b * HW + p] = o;
        }
    }
}

// bf16 NHWC [B][H][W][3] -> bf16 [B][H][W][4]
__global__ __launch_bounds__(256) void stem_pack_bf16_kernel(const __bf16* __restrict__ x, bf16x4* __restrict__ x4, long n) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    bf16x4 o;
    o[0] = x[p * 3];
    o[1] = x[p * 3 + 1];
    o[2] = x[p * 3 + 2];
    o[3] = (__bf16)0.f;
    x4[p] = o;
}

// fp32 OIHW [64][3][7][7] -> bf16 [kb][o][32] for the forward: column 32*kb + kk is k = (c*7 + ky)*7 + kx, the order of the OIHW tensor (and of the
// patch matrix of stem.hip), zero from k = 147 up
__global__ __launch_bounds__(256) void stem_pack_weight_kernel(const float* __restrict__ w, __bf16* __restrict__ wp) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= SD_KB * 64 * 32) return;
    const int kk = i & 31, o = (i >> 5) & 63, kb = i >> 11;
    const int k = kb * 32 + kk;
    wp[i] = (__bf16)(k < 147 ? w[o * 147 + k] : 0.f);
}

// Staging of ROWS image rows (first row h0) x SD_ROWPX pixels (first column c0) of image `img` into LDS, zero outside the image, in two halves: every
// load is issued before the first LDS write, and the weight gradient issues the next tile's loads before it computes on the current one.
template <int ROWS>
struct ImageRows {
    static constexpr int N = (ROWS * SD_ROWPX + 255) / 256;
    uint2 v[N];
    __device__ __forceinline__ void load(const uint2* __restrict__ img, int h0, int c0, int H, int W, int tid) {
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const int i = tid + j * 256;
            const int r = i / SD_ROWPX, c = i - r * SD_ROWPX;
            const int h = h0 + r, w = c0 + c;
            v[j] = make_uint2(0u, 0u);
            if (i < ROWS * SD_ROWPX && (unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W) v[j] = img[(long)h * W + w];
        }
    }
    __device__ __forceinline__ void store(uint2* sx, int tid) const {
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const int i = tid + j * 256;
            if (i < ROWS * SD_ROWPX) sx[i] = v[j];
        }
    }
};

// ---- forward ----------------------------------------------------------------------------------------------------------------------------------
// Workgroup = one tile of 8 output rows x 64 output columns of one image; wave w computes rows 2w, 2w + 1.  The weights are the A operand (row =
// output channel) and live in registers for the whole tile; the B operand (column = output pixel) is gathered from the staged image rows.
// The contraction runs in EXACTLY the order of the patch-matrix GEMM it replaces (igemm_nt.hip on the 192-column matrix of stem.hip): six K = 32
// steps over k = (c*7 + ky)*7 + kx in ascending order, element 8q + j of a step in lane quarter q, zeros from k = 147 up, the all-zero sixth step
// included - so every fp32 sum, and with it y, has the bits of that route (tests/test_gpu_stem_direct.py asserts it).  Element k of output pixel
// (ho, wo) is the bf16 at staged row 2*(ho - ho0) + ky, pixel 2*(wo - wo0) + kx, channel c: a lane keeps its 40 (ky, kx, c) byte offsets in
// registers and builds a fragment from eight 2-byte LDS reads.  Nothing outside the 7x7x3 window is ever read, so a NaN next to a window stays
// out of it.  A-tile `ot` row r holds output channel (r >> 2)*16 + ot*4 + (r & 3), so that a lane's 16 results are 16 consecutive channels of
// one pixel (two 16-byte stores) and a wave stores 2 KiB contiguous per 16 pixels.
struct StemFwdParams {
    const uint2* x4;
    const bf16x8* wp;
    __bf16* y;
    int B, H, W, Ho, Wo, tiles_x, tiles_y;
};

__global__ __launch_bounds__(256, 2) void stem_direct_fwd_kernel(StemFwdParams p) {
    __shared__ __attribute__((aligned(16))) uint2 sx[SD_FWD_ROWS * SD_ROWPX];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tx = blockIdx.x % p.tiles_x, ty = (blockIdx.x / p.tiles_x) % p.tiles_y, b = blockIdx.x / (p.tiles_x * p.tiles_y);
    const int wo0 = tx * SD_TW, ho0 = ty * SD_FWD_TH;
    ImageRows<SD_FWD_ROWS> rows;
    rows.load(p.x4 + (long)b * p.H * p.W, 2 * ho0 - 3, 2 * wo0 - 3, p.H, p.W, tid);

    const int col = lane & 15, q = lane >> 4;
    bf16x8 wf[SD_KB - 1][4];                       // the sixth step's weights are zeros
#pragma unroll
    for (int kb = 0; kb < SD_KB - 1; ++kb)
#pragma unroll
        for (int ot = 0; ot < 4; ++ot) wf[kb][ot] = p.wp[(kb * 64 + (col >> 2) * 16 + ot * 4 + (col & 3)) * 4 + q];
    int off[SD_KB - 1][8];                         // byte offset of window element k = 32*kb + 8*q + j from the window's first pixel; -1: k >= 147
#pragma unroll
    for (int kb = 0; kb < SD_KB - 1; ++kb)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = kb * 32 + q * 8 + j;
            const int c = k / 49, r = k - c * 49, ky = r / 7, kx = r - ky * 7;
            off[kb][j] = k < 147 ? ky * SD_ROWB + kx * 8 + c * 2 : -1;
        }
    rows.store(sx, tid);
    __syncthreads();

    const char* sxb = reinterpret_cast<const char*>(sx);
    bf16x8 zero8;
#pragma unroll
    for (int e = 0; e < 8; ++e) zero8[e] = (__bf16)0.f;
    for (int rr = wave * 2; rr < wave * 2 + 2; ++rr) {
        const int ho = ho0 + rr;
        if (ho >= p.Ho) break;
        for (int mt = 0; mt < 4; ++mt) {
            if (wo0 + mt * 16 >= p.Wo) break;
            const char* win = sxb + 2 * rr * SD_ROWB + 16 * (mt * 16 + col);       // first pixel of this lane's window
            f32x4 acc[4];
#pragma unroll
            for (int ot = 0; ot < 4; ++ot) acc[ot] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kb = 0; kb < SD_KB - 1; ++kb) {
                union { bf16x8 v; unsigned short s[8]; } f;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    if (kb < 4) {
                        f.s[j] = *reinterpret_cast<const unsigned short*>(win + off[kb][j]);
                    } else {
                        const unsigned short v = *reinterpret_cast<const unsigned short*>(win + (off[kb][j] < 0 ? 0 : off[kb][j]));
                        f.s[j] = off[kb][j] < 0 ? (unsigned short)0 : v;
                    }
                }
#pragma unroll
                for (int ot = 0; ot < 4; ++ot) acc[ot] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[kb][ot], f.v, acc[ot], 0, 0, 0);
            }
#pragma unroll
            for (int ot = 0; ot < 4; ++ot) acc[ot] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(zero8, zero8, acc[ot], 0, 0, 0);      // k = 160 .. 191
            const int wo = wo0 + mt * 16 + col;
            if (wo < p.Wo) {
                bf16x8 o0, o1;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    o0[e] = (__bf16)acc[0][e];
                    o0[4 + e] = (__bf16)acc[1][e];
                    o1[e] = (__bf16)acc[2][e];
                    o1[4 + e] = (__bf16)acc[3][e];
                }
                bf16x8* dst = reinterpret_cast<bf16x8*>(p.y + (((long)b * p.Ho + ho) * p.Wo + wo) * 64 + q * 16);
                dst[0] = o0;
                dst[1] = o1;
            }
        }
    }
}

// ---- weight gradient --------------------------------------------------------------------------------------------------------------------------
// Transposed LDS read on a raw LDS byte address (the form and the explicit waits of igemm_tn.hip:36-47).  Per 16-lane group it reads 4 rows x 16
// columns of bf16 and hands lane i column i of the 4 rows; lane 4r + c of the group supplies the address of row r, columns 4c .. 4c+3.
template <int OFF>
__device__ __forceinline__ s16x4 sd_tr_read(unsigned lds_addr) {
    s16x4 v;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(lds_addr), "n"(OFF));
    return v;
}

__device__ __forceinline__ unsigned sd_lds_address(const void* generic_ptr_into_lds) {
    return (unsigned)(uintptr_t)((__attribute__((address_space(3))) const char*)generic_ptr_into_lds);
}

struct StemWgradParams {
    const uint2* x4;
    const bf16x8* dy;
    float* part;
    int B, H, W, Ho, Wo, tiles_x, tiles_y, tiles, S;
    // POOL: dy is not in memory; it is built per tile from the pooled gradient, the argmax bytes and the BatchNorm scale
    const bf16x8* dpool;
    const uint2* idx;
    const float* scale;
    int Hp, Wp;
};

// POOL staging: the patch of dpool [B,Hp,Wp,64] and of the argmax bytes that a tile's dy is built from, SD_PP_ROWS x SD_PP_COLS pooled pixels from
// (hp0, wp0) = (ho0 / 2, wo0 / 2).  It travels in registers like the image rows; store() packs the 8 argmax bytes of an item into 8 nibbles (a byte
// above 15 becomes 15: like every byte above 8 it matches no tap), and pooled pixels outside the map get nibble 15 everywhere.
struct PoolPatch {
    static constexpr int N = (SD_PP_ITEMS + 255) / 256;
    bf16x8 g[N];
    uint2 ib[N];
    __device__ __forceinline__ void load(const bf16x8* __restrict__ dpool, const uint2* __restrict__ idx, int b, int hp0, int wp0, int Hp, int Wp, int tid) {
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const int i = tid + j * 256;
            const int c = i & 7, px = i >> 3;
            const int pr = px / SD_PP_COLS, pc = px - pr * SD_PP_COLS;
            const int hp = hp0 + pr, wp = wp0 + pc;
#pragma unroll
            for (int e = 0; e < 8; ++e) g[j][e] = (__bf16)0.f;
            ib[j] = make_uint2(~0u, ~0u);
            if (i < SD_PP_ITEMS && hp < Hp && wp < Wp) {
                const long off = (((long)b * Hp + hp) * Wp + wp) * 8 + c;
                g[j] = dpool[off];
                ib[j] = idx[off];
            }
        }
    }
    static __device__ __forceinline__ unsigned nibbles(unsigned x) {          // 4 bytes -> 4 nibbles in the low 16 bits
        unsigned t = (x >> 4) & 0x0f0f0f0fu;                                    // bit 0 of each byte of t: the byte of x is above 15
        t |= t >> 1;
        t |= t >> 2;
        x = (x & 0x0f0f0f0fu) | ((t & 0x01010101u) * 15u);
        x = (x | (x >> 4)) & 0x00ff00ffu;
        return (x | (x >> 8)) & 0xffffu;
    }
    __device__ __forceinline__ void store(bf16x8* sdp, unsigned* sidx, int tid) const {
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const int i = tid + j * 256;
            if (i < SD_PP_ITEMS) {
                sdp[i] = g[j];
                sidx[i] = nibbles(ib[j].x) | (nibbles(ib[j].y) << 16);
            }
        }
    }
};

// Workgroup s walks tiles [s*tiles/S, (s+1)*tiles/S) of 4 output rows x 64 output columns and keeps dw[64][7][32] in the accumulators of its four
// waves: wave (kt = wave & 1, oh = wave >> 1) owns channels 32*oh .. 32*oh+31 and k = 16*kt .. 16*kt+15.  One MFMA contracts 32 pixels of one
// output row; with g = lane >> 4, MFMA k index 8g + j is pixel 16*(j >> 2) + 4g + (j & 3) of the 32 on BOTH operands.
//   dy operand (A, row = channel): the staged dy rows [pixel][64 channels], 16-byte chunk c of pixel P at physical chunk c ^ (P & 7): the 8
//     consecutive pixels of a 32-lane half then cover 64 distinct banks.
//   x operand (B, column = k): the staged image row; pixel P's patch row is the 64 bytes at 16*P, so a half reads one span of 144 bytes.
// Pixels past Wo: their dy is staged as zero and their x fragment elements are zeroed too (the image there can hold anything, 0 * NaN is NaN);
// rows past Ho are skipped.
// POOL (mi_stem_conv_wgrad_pool): the staged dy rows are not loaded but built, between two barriers of their own, from the staged patch of the
// pooled gradient - the max-pool / ReLU / BatchNorm backward of stem_pool_bwd_kernel (stem.hip) per (pixel, 8-channel chunk) item, with the same
// <= 4 windows in the same (ho, wo) order, fp32 accumulation and (__bf16)(acc * scale[c]): the staged rows, and with them dw, have the bits of that
// kernel's dy, which is then never written (152 MB at B = 8, 769 x 769) nor read back.
template <bool POOL>
__global__ __launch_bounds__(256, 2) void stem_direct_wgrad_kernel(StemWgradParams p) {
    __shared__ __attribute__((aligned(16))) uint2 sx[SD_WG_ROWS * SD_ROWPX];
    __shared__ __attribute__((aligned(16))) bf16x8 sdy[SD_WG_TH * SD_TW * 8];
    __shared__ __attribute__((aligned(16))) bf16x8 sdp[POOL ? SD_PP_ITEMS : 1];
    __shared__ unsigned sidx[POOL ? SD_PP_ITEMS : 1];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kt = wave & 1, oh = wave >> 1;
    const int s = blockIdx.x;
    const int t_begin = (int)((long)s * p.tiles / p.S), t_end = (int)((long)(s + 1) * p.tiles / p.S);
    const int g = lane >> 4, rq = (lane & 15) >> 2, pc = lane & 3;
    const int pix = 4 * g + rq;                                  // the pixel (of the first 16 of a step) whose address this lane supplies
    const unsigned sx_base = sd_lds_address(sx) + 16 * pix + 32 * kt + 8 * pc;
    const unsigned sdy_base = sd_lds_address(sdy) + 128 * pix + 8 * (pc & 1);
    const int sw = pix & 7;                                      // (pix + 16, + 32, + 48 have the same low bits)

    f32x4 acc[2][7];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int ky = 0; ky < 7; ++ky) acc[a][ky] = f32x4{0.f, 0.f, 0.f, 0.f};

    // the next tile's image rows and dy rows travel in registers while the current tile is contracted
    ImageRows<SD_WG_ROWS> nx;
    bf16x8 ny[POOL ? 1 : 8];
    PoolPatch np;
    float sc[8];                                                 // POOL: the BatchNorm scale of this thread's 8 channels (chunk tid & 7 of every item)
    if constexpr (POOL) {
#pragma unroll
        for (int e = 0; e < 8; ++e) sc[e] = p.scale[(tid & 7) * 8 + e];
    }
    auto load_tile = [&](int t) {
        const int tx = t % p.tiles_x, ty = (t / p.tiles_x) % p.tiles_y, b = t / (p.tiles_x * p.tiles_y);
        const int wo0 = tx * SD_TW, ho0 = ty * SD_WG_TH;
        nx.load(p.x4 + (long)b * p.H * p.W, 2 * ho0 - 3, 2 * wo0 - 3, p.H, p.W, tid);
        if constexpr (POOL) {
            np.load(p.dpool, p.idx, b, ho0 >> 1, wo0 >> 1, p.Hp, p.Wp, tid);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int i = tid + j * 256;
                const int c = i & 7, P = (i >> 3) & 63, rr = i >> 9;
                const int ho = ho0 + rr, wo = wo0 + P;
#pragma unroll
                for (int e = 0; e < 8; ++e) ny[j][e] = (__bf16)0.f;
                if (ho < p.Ho && wo < p.Wo) ny[j] = p.dy[(((long)b * p.Ho + ho) * p.Wo + wo) * 8 + c];
            }
        }
    };
    load_tile(t_begin);
    for (int t = t_begin; t < t_end; ++t) {
        const int tx = t % p.tiles_x, ty = (t / p.tiles_x) % p.tiles_y;
        const int wo0 = tx * SD_TW, ho0 = ty * SD_WG_TH;
        __syncthreads();                                         // the previous tile's fragment reads are done
        nx.store(sx, tid);
        if constexpr (POOL) {
            np.store(sdp, sidx, tid);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int i = tid + j * 256;
                const int c = i & 7, P = (i >> 3) & 63, rr = i >> 9;
                sdy[(rr * SD_TW + P) * 8 + (c ^ (P & 7))] = ny[j];
            }
        }
        __syncthreads();
        if (t + 1 < t_end) load_tile(t + 1);
        if constexpr (POOL) {
            // item j of this thread: conv row rr = j >> 1, column P, chunk c - the items of the plain staging above.  Conv row ho0 + rr (ho0 even) lies in
            // the windows of pooled rows (rr >> 1) .. ((rr + 1) >> 1) of the patch at kernel row rr - 2*hl + 1, and likewise along the columns.
            const int c = tid & 7;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int rr = j >> 1, P = (tid >> 3) + 32 * (j & 1);
                bf16x8 o;
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = (__bf16)0.f;
                if (ho0 + rr < p.Ho && wo0 + P < p.Wo) {
                    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int hl = rr >> 1; hl <= ((rr + 1) >> 1); ++hl) {
                        const int ky = rr - 2 * hl + 1;
                        for (int wl = P >> 1; wl <= ((P + 1) >> 1); ++wl) {
                            const unsigned tap = (unsigned)(ky * 3 + (P - 2 * wl + 1));
                            const int it = (hl * SD_PP_COLS + wl) * 8 + c;
                            const bf16x8 gv = sdp[it];
                            const unsigned nib = sidx[it];
#pragma unroll
                            for (int e = 0; e < 8; ++e)
                                if (((nib >> (4 * e)) & 15u) == tap) a[e] += (float)gv[e];
                        }
                    }
#pragma unroll
                    for (int e = 0; e < 8; ++e) o[e] = (__bf16)(a[e] * sc[e]);
                }
                sdy[(rr * SD_TW + P) * 8 + (c ^ (P & 7))] = o;
            }
            __syncthreads();
        }
        const int nrows = min(SD_WG_TH, p.Ho - ho0);
        for (int rr = 0; rr < nrows; ++rr) {
#pragma unroll
            for (int step = 0; step < 2; ++step) {
                const int left = p.Wo - (wo0 + step * 32);       // live pixels of this step (wave-uniform)
                if (left <= 0) break;
                union { bf16x8 v; s16x4 h[2]; uint64_t d[2]; } yf[2], xf[7];
                const unsigned ya = sdy_base + rr * SD_DYROWB + step * 32 * 128;
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    const unsigned addr = ya + (((2 * (oh * 2 + a) + (pc >> 1)) ^ sw) << 4);
                    yf[a].h[0] = sd_tr_read<0>(addr);
                    yf[a].h[1] = sd_tr_read<16 * 128>(addr);
                }
                const unsigned xa = sx_base + 2 * rr * SD_ROWB + step * 32 * 16;
#pragma unroll
                for (int ky = 0; ky < 7; ++ky) {
                    xf[ky].h[0] = sd_tr_read<0>(xa + ky * SD_ROWB);
                    xf[ky].h[1] = sd_tr_read<16 * 16>(xa + ky * SD_ROWB);
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_sched_barrier(0);
                if (left < 32) {
                    // element e of half h is pixel 16h + 4g + e of the step
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int nv = left - (16 * h + 4 * g);
                        const uint64_t m = nv >= 4 ? ~0ull : (nv <= 0 ? 0ull : ((1ull << (16 * nv)) - 1ull));
#pragma unroll
                        for (int ky = 0; ky < 7; ++ky) xf[ky].d[h] &= m;
                    }
                }
#pragma unroll
                for (int ky = 0; ky < 7; ++ky)
#pragma unroll
                    for (int a = 0; a < 2; ++a) acc[a][ky] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yf[a].v, xf[ky].v, acc[a][ky], 0, 0, 0);
            }
        }
    }
    // D: column (lane & 15) = k, row 4*(lane >> 4) + e = channel within the 16
    float* dst = p.part + (long)s * SD_PART;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int ky = 0; ky < 7; ++ky)
#pragma unroll
            for (int e = 0; e < 4; ++e) dst[(((oh * 2 + a) * 16 + 4 * g + e) * 7 + ky) * 32 + kt * 16 + (lane & 15)] = acc[a][ky][e];
}

// dw[o][c][ky][kx] = sum over the S partials, in ascending split order (bitwise reproducible); thread = one (o, ky, k) of the partial layout, so a
// wave's loads are 256 contiguous bytes; k with c = 3 or kx >= 7 is dropped.
__global__ __launch_bounds__(256) void stem_direct_wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw, int S) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= SD_PART) return;
    const int k = i & 31, ky = (i >> 5) % 7, o = i / 224;
    const int kx = k >> 2, c = k & 3;
    if (c == 3 || kx >= 7) return;
    float sum = 0.f;
    int s = 0;
    for (; s + 64 <= S; s += 64) {                               // 64 loads in flight, added in ascending order
        float v[64];
#pragma unroll
        for (int j = 0; j < 64; ++j) v[j] = part[(long)(s + j) * SD_PART + i];
#pragma unroll
        for (int j = 0; j < 64; ++j) sum += v[j];
    }
    for (; s < S; ++s) sum += part[(long)s * SD_PART + i];
    dw[((o * 3 + c) * 7 + ky) * 7 + kx] = sum;
}

int stem_wgrad_splits(int B, int Ho, int Wo) {
    const long tiles = (long)B * ((Ho + SD_WG_TH - 1) / SD_WG_TH) * ((Wo + SD_TW - 1) / SD_TW);
    const long slots = mi_sw().stem_wgrad_splits;
    return (int)(tiles < slots ? tiles : slots);
}

// the geometry every entry point insists on: a 7x7 / stride 2 / pad 3 conv, every element offset within 32 bits
const char* stem_direct_geometry(int B, int H, int W, int Ho, int Wo) {
    if (B <= 0 || H <= 0 || W <= 0) return "B, H, W must be positive";
    if (Ho != (H + 6 - 7) / 2 + 1 || Wo != (W + 6 - 7) / 2 + 1) return "output size must be that of a 7x7/2/3 conv";
    if ((long)B * H * W * 4 >= (1l << 31) || (long)B * Ho * Wo * 64 >= (1l << 31)) return "tensor exceeds the 32-bit offset range";
    return nullptr;
}

}  // namespace

extern "C" int mi_stem_direct_enabled(void) { return mi_sw().stem_direct != 0; }

extern "C" int mi_stem_pack_image(const void* x, int x_is_bf16_nhwc, void* x4, int B, int H, int W, void* stream) {
    MI_REQUIRE(x && x4 && B > 0 && H > 0 && W > 0, "mi_stem_pack_image: bad argument");
    MI_REQUIRE(x_is_bf16_nhwc == 0 || x_is_bf16_nhwc == 1, "mi_stem_pack_image: x_is_bf16_nhwc=%d (0: fp32 NCHW, 1: bf16 NHWC)", x_is_bf16_nhwc);
    MI_REQUIRE((reinterpret_cast<uintptr_t>(x4) & 7) == 0 && (reinterpret_cast<uintptr_t>(x) & (x_is_bf16_nhwc ? 1 : 3)) == 0, "mi_stem_pack_image: alignment");
    MI_REQUIRE((long)B * H * W * 4 < (1l << 31), "mi_stem_pack_image: tensor exceeds the 32-bit offset range");
    MI_REQUIRE(B < 65536, "mi_stem_pack_image: B = %d exceeds the grid", B);
    const long HW = (long)H * W;
    if (x_is_bf16_nhwc)
        hipLaunchKernelGGL(stem_pack_bf16_kernel, dim3((unsigned)((B * HW + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const __bf16*)x, (bf16x4*)x4,
                           B * HW);
    else
        hipLaunchKernelGGL(stem_pack_f32_kernel, dim3((unsigned)((HW + 1023) / 1024), (unsigned)B), dim3(256), 0, (hipStream_t)stream, (const float*)x,
                           (bf16x4*)x4, HW, B);
    MI_CHECK_LAUNCH("mi_stem_pack_image");
    return MI_OK;
}

extern "C" int mi_stem_conv_fwd(const void* x4, const float* w, void* wpack, void* y, int B, int H, int W, int O, int Ho, int Wo, void* stream) {
    MI_REQUIRE(x4 && w && wpack && y, "mi_stem_conv_fwd: null operand");
    MI_REQUIRE(O == 64, "mi_stem_conv_fwd: O=%d (the stem has 64 output channels)", O);
    const char* bad = stem_direct_geometry(B, H, W, Ho, Wo);
    MI_REQUIRE(!bad, "mi_stem_conv_fwd: %s", bad);
    MI_REQUIRE((reinterpret_cast<uintptr_t>(x4) & 7) == 0 && mi_aligned16(wpack) && mi_aligned16(y), "mi_stem_conv_fwd: alignment");
    hipLaunchKernelGGL(stem_pack_weight_kernel, dim3(SD_KB * 64 * 32 / 256), dim3(256), 0, (hipStream_t)stream, w, (__bf16*)wpack);
    MI_CHECK_LAUNCH("mi_stem_conv_fwd (weight pack)");
    StemFwdParams p;
    p.x4 = (const uint2*)x4;
    p.wp = (const bf16x8*)wpack;
    p.y = (__bf16*)y;
    p.B = B, p.H = H, p.W = W, p.Ho = Ho, p.Wo = Wo;
    p.tiles_x = (Wo + SD_TW - 1) / SD_TW;
    p.tiles_y = (Ho + SD_FWD_TH - 1) / SD_FWD_TH;
    hipLaunchKernelGGL(stem_direct_fwd_kernel, dim3((unsigned)(B * p.tiles_x * p.tiles_y)), dim3(256), 0, (hipStream_t)stream, p);
    MI_CHECK_LAUNCH("mi_stem_conv_fwd");
    return MI_OK;
}

extern "C" size_t mi_stem_conv_wgrad_workspace(int B, int Ho, int Wo) {
    if (B <= 0 || Ho <= 0 || Wo <= 0) return 0;
    return (size_t)stem_wgrad_splits(B, Ho, Wo) * SD_PART * sizeof(float);
}

namespace {
// both weight-gradient entries: pool false -> dy from memory; true -> dy built in the launch from (dpool, idx, scale)
int stem_wgrad_launch(const char* who, bool pool, const void* dy, const void* dpool, const uint8_t* idx, const float* scale, const void* x4, float* dw, int B,
                      int H, int W, int O, int Ho, int Wo, int Hp, int Wp, void* workspace, size_t workspace_bytes, void* stream) {
    MI_REQUIRE((pool ? dpool && idx && scale : dy != nullptr) && x4 && dw && workspace, "%s: null operand", who);
    MI_REQUIRE(O == 64, "%s: O=%d (the stem has 64 output channels)", who, O);
    const char* bad = stem_direct_geometry(B, H, W, Ho, Wo);
    MI_REQUIRE(!bad, "%s: %s", who, bad);
    MI_REQUIRE(!pool || (Hp == (Ho + 2 - 3) / 2 + 1 && Wp == (Wo + 2 - 3) / 2 + 1), "%s: pooled size must be that of a 3x3/2/1 max-pool of the conv output", who);
    MI_REQUIRE((reinterpret_cast<uintptr_t>(x4) & 7) == 0 && mi_aligned16(workspace) && (reinterpret_cast<uintptr_t>(dw) & 3) == 0 &&
                   (pool ? mi_aligned16(dpool) && (reinterpret_cast<uintptr_t>(idx) & 7) == 0 && (reinterpret_cast<uintptr_t>(scale) & 3) == 0 : mi_aligned16(dy)),
               "%s: alignment", who);
    MI_REQUIRE(workspace_bytes >= mi_stem_conv_wgrad_workspace(B, Ho, Wo), "%s: workspace holds %zu bytes, %zu needed", who, workspace_bytes,
               mi_stem_conv_wgrad_workspace(B, Ho, Wo));
    StemWgradParams p;
    p.x4 = (const uint2*)x4;
    p.dy = (const bf16x8*)dy;
    p.dpool = (const bf16x8*)dpool;
    p.idx = (const uint2*)idx;
    p.scale = scale;
    p.Hp = Hp, p.Wp = Wp;
    p.part = (float*)workspace;
    p.B = B, p.H = H, p.W = W, p.Ho = Ho, p.Wo = Wo;
    p.tiles_x = (Wo + SD_TW - 1) / SD_TW;
    p.tiles_y = (Ho + SD_WG_TH - 1) / SD_WG_TH;
    p.tiles = B * p.tiles_x * p.tiles_y;
    p.S = stem_wgrad_splits(B, Ho, Wo);
    if (!pool)
        hipLaunchKernelGGL(stem_direct_wgrad_kernel<false>, dim3((unsigned)p.S), dim3(256), 0, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(stem_direct_wgrad_kernel<true>, dim3((unsigned)p.S), dim3(256), 0, (hipStream_t)stream, p);
    MI_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(stem_direct_wgrad_reduce_kernel, dim3(SD_PART / 256), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, dw, p.S);
    MI_CHECK_LAUNCH(who);
    return MI_OK;
}
}  // namespace

extern "C" int mi_stem_conv_wgrad(const void* dy, const void* x4, float* dw, int B, int H, int W, int O, int Ho, int Wo, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    return stem_wgrad_launch("mi_stem_conv_wgrad", false, dy, nullptr, nullptr, nullptr, x4, dw, B, H, W, O, Ho, Wo, 0, 0, workspace, workspace_bytes, stream);
}

extern "C" int mi_stem_pool_wgrad_enabled(void) { return mi_sw().stem_pool_wgrad != 0; }

extern "C" int mi_stem_conv_wgrad_pool(const void* dpool, const uint8_t* idx, const float* scale, const void* x4, float* dw, int B, int H, int W, int O,
                                       int Ho, int Wo, int Hp, int Wp, void* workspace, size_t workspace_bytes, void* stream) {
    return stem_wgrad_launch("mi_stem_conv_wgrad_pool", true, nullptr, dpool, idx, scale, x4, dw, B, H, W, O, Ho, Wo, Hp, Wp, workspace, workspace_bytes, stream);
}
