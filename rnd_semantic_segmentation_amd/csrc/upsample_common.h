// What the bilinear-upsample sources (upsample_ce.hip, upsample_lovasz.hip, upsample_infer.hip, upsample_slide.hip, fada.hip, classmix.hip) share: the source-index arithmetic, the fixed-order reductions,
// the per-pixel softmax core, the per-pixel probabilities and prediction of the inference tails, the prologue / pixel / epilogue helpers of the two kernel skeletons of the fused upsample + loss heads (x-tile and row-walk), the LDS layout of the first,
// and the launch planning.  Everything is file-local to the source that includes it (anonymous namespace): kernel names do not change.
#pragma once
#include "mi_common.h"
#include <cmath>
#include <type_traits>

namespace {

constexpr int KMAX = 32;            // classes held in registers
constexpr int JT = 32;              // low-res columns of the largest x-tile; the launcher narrows it for large upsample factors (pick_jt)
constexpr int GDL_XT = 256;         // output pixels of one row per workgroup in the row-walk kernels: one per thread and row

struct Axis {              // source index exactly as ATen computes it in fp32: align_corners (off = 0): scale * dst; otherwise (off = 0.5):
    float scale, off;      // max(scale * (dst + 0.5) - 0.5, 0)  (adding / subtracting 0.0f is exact: the align_corners bits are unchanged)
    int n_in, n_out;
    __device__ __forceinline__ float srcf(int dst) const {
        const float f = scale * ((float)dst + off) - off;
        return f < 0.f ? 0.f : f;
    }
    __device__ __forceinline__ void src(int dst, int& i0, int& i1, float& lam) const {
        const float f = srcf(dst);
        i0 = (int)f;
        if (i0 > n_in - 1) i0 = n_in - 1;
        i1 = (i0 < n_in - 1) ? i0 + 1 : i0;
        lam = f - (float)i0;
    }
    // first dst index whose i0 >= c  (n_out if none)
    __device__ __forceinline__ int first_with_i0_ge(int c) const {
        if (c <= 0) return 0;
        if (scale <= 0.f) return n_out;
        if (c > n_in - 1) return n_out;
        int d = (int)((float)c / scale) - 2;
        if (d < 0) d = 0;
        if (d > n_out) d = n_out;
        while (d < n_out) {
            int i0 = (int)srcf(d);
            if (i0 > n_in - 1) i0 = n_in - 1;
            if (i0 >= c) break;
            ++d;
        }
        return d;
    }
};

inline Axis make_axis(int n_in, int n_out, int align_corners = 1) {
    Axis a;
    a.n_in = n_in;
    a.n_out = n_out;
    a.off = align_corners ? 0.f : 0.5f;
    a.scale = align_corners ? ((n_out > 1) ? (float)(n_in - 1) / (float)(n_out - 1) : 0.f) : (float)n_in / (float)n_out;      // (a size was given: in / out)
    return a;
}

// (1 - l) a + l b from two rounded products, whatever the compiler would contract at the call site: what two kernels that have to agree bit for bit
// (the passes of the Lovasz head) interpolate with.
__device__ __forceinline__ float lerp_rounded(float l, float a, float b) {
#pragma clang fp contract(off)
    const float pa = (1.f - l) * a, pb = l * b;
    return pa + pb;
}

__device__ __forceinline__ float lerp2(float v00, float v01, float v10, float v11, float lx, float ly) {
    return (1.f - ly) * ((1.f - lx) * v00 + lx * v01) + ly * ((1.f - lx) * v10 + lx * v11);
}

__device__ __forceinline__ void block_sum2(float& a, float& b, float* red) {
    // fixed-order tree over 256 threads
    const int t = threadIdx.x;
    red[t] = a;
    red[256 + t] = b;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) {
            red[t] += red[t + w];
            red[256 + t] += red[256 + t + w];
        }
        __syncthreads();
    }
    a = red[0];
    b = red[256];
    __syncthreads();
}

__device__ __forceinline__ float wave_sum(float v) {          // xor butterfly: both partners add the same two values, every lane ends with the same bits
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ unsigned wave_sum(unsigned v) {
    for (int m = 32; m > 0; m >>= 1) v += (unsigned)__shfl_xor((int)v, m);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// ------------------------------------------------------------------------------------------------ the per-pixel softmax core
// KT > 0: the class count is a compile-time constant (19 for Cityscapes: exact-length register loops instead of 32 predicated iterations);
// KT == 0: K is read from the arguments.  kreg<KT>: the register array length.
template <int KT>
constexpr int kreg = KT > 0 ? KT : KMAX;

struct NoTerm {
    __device__ __forceinline__ void operator()(int, float) const {}
};

// v[k] = exp(v[k] - mx) for k < K; returns their sum.  PICK: *picked = v[lab] - mx taken BEFORE the exponential (exp() of it underflows to 0 for a
// confidently wrong pixel, |logit| gap > 87, and log(0) would make a loss inf).  term(k, v[k] - mx) sees every class, before the exponential too.
// kr is the length of the register array v (kreg<KT>).  It arrives as an argument, and v as a pointer, on purpose: as `float (&v)[KR]` with the length
// a template parameter, or with v declared in a function below the kernel, the generic instantiations of the kernels (32 predicated iterations) compiled
// to five times the instructions and spilled (measured; profiles/upsample_skeleton_resources.txt).  So v and the loops after the core stay in the kernel.
template <bool PICK = false, class Term = NoTerm>
__device__ __forceinline__ float exp_terms(float* v, int kr, float mx, int K, long lab = 0, float* picked = nullptr, Term term = Term()) {
    float se = 0.f;
    if constexpr (PICK) *picked = 0.f;
#pragma unroll
    for (int k = 0; k < kr; ++k) {
        if (k < K) {
            if constexpr (PICK) {
                if (k == lab) *picked = v[k] - mx;
            }
            term(k, v[k] - mx);
            v[k] = __expf(v[k] - mx);
            se += v[k];
        }
    }
    return se;
}

// The K logits of one output pixel interpolated from two staged columns (c0, c1: already interpolated along y), then exp_terms on them.
template <bool PICK = false, class Term = NoTerm>
__device__ __forceinline__ float softmax_terms(const float* c0, const float* c1, float lx, int K, float* v, int kr, long lab = 0, float* picked = nullptr,
                                               Term term = Term()) {
    float mx = -3.0e38f;
#pragma unroll
    for (int k = 0; k < kr; ++k) {
        if (k < K) {
            v[k] = (1.f - lx) * c0[k] + lx * c1[k];
            mx = fmaxf(mx, v[k]);
        }
    }
    return exp_terms<PICK>(v, kr, mx, K, lab, picked, term);
}

// ------------------------------------------------------------------------------------------------ the per-pixel probabilities of the inference tails
// Shared by the inference tails of upsample_infer.hip and the self-training pass of classmix.hip, so that the pseudo-labels written during
// evaluation and those drawn inside a training step cannot drift apart.
// The per-source arithmetic: the bilinear (align_corners) sample of the NHWC map `low` (one image) at output pixel
// (y, x), then v[k] = exp(value - max); returns 1 / sum (the probabilities are v[k] * result) and the first arg max.
// The interpolation is written out operation by operation - row0 = fma(lx, v01, (1-lx) v00), row1 = fma(1-lx, v10, lx v11),
// value = (1-ly) row0 + ly row1 with both products rounded - because that is the order mi_upsample_softmax has always computed (what the
// compiler's contraction made of lerp2 there) and two kernels have to agree on it bit for bit; contraction is off so that it stays put.
template <int KR>
__device__ __forceinline__ float interp_softmax_terms(const float* __restrict__ low, int K, const Axis& ay, const Axis& ax, int y, int x,
                                                      float (&v)[KR], int& arg) {
#pragma clang fp contract(off)
    const int w = ax.n_in;
    int y0, y1, x0, x1;
    float ly, lx;
    ay.src(y, y0, y1, ly);
    ax.src(x, x0, x1, lx);
    const float* p00 = low + ((long)y0 * w + x0) * K;
    const float* p01 = low + ((long)y0 * w + x1) * K;
    const float* p10 = low + ((long)y1 * w + x0) * K;
    const float* p11 = low + ((long)y1 * w + x1) * K;
    const float mlx = 1.f - lx, mly = 1.f - ly;
    float mx = -3.0e38f;
    arg = 0;
#pragma unroll
    for (int k = 0; k < KR; ++k) {
        if (k < K) {
            const float row0 = __builtin_fmaf(lx, p01[k], mlx * p00[k]);
            const float row1 = __builtin_fmaf(mlx, p10[k], lx * p11[k]);
            v[k] = mly * row0 + ly * row1;
            if (v[k] > mx) {
                mx = v[k];
                arg = k;
            }
        }
    }
    return 1.f / exp_terms(v, KR, mx, K);
}

struct ProbSrc {
    const float* low;
    Axis ay, ax;
    int mirror;
};
constexpr int MAX_PROB_SRC = 16;
struct ProbSrcs {
    ProbSrc s[MAX_PROB_SRC];      // by value in the kernel arguments: no device table
};

__device__ __forceinline__ float add_rounded_product(float acc, float a, float b) {
#pragma clang fp contract(off)
    const float p = a * b;
    return acc + p;
}

// The per-pixel arithmetic of the multi-scale tails, shared by the probability kernel, the predict-and-score kernel and the ClassMix pass so that
// they cannot drift apart: acc[p][k] = ((p_0 + ... + p_{n-1}) / div_a) / div_b for the P pixels (y, xb .. xb+P-1), summed in source order from
// rounded products, with true divisions (the second one skipped when div_b == 1).  s_all: the n sources.
template <int KR, int P>
__device__ __forceinline__ void multi_probs(const ProbSrc* s_all, int n, int K, int W, int y, int xb, float div_a, float div_b, float (&acc)[P][KR]) {
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
        for (int k = 0; k < KR; ++k) acc[p][k] = 0.f;      // 0 + p_0 == p_0 exactly (p_0 >= +0)
    for (int i = 0; i < n; ++i) {
        const ProbSrc& s = s_all[i];
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const int x = xb + p;
            float v[KR];
            int arg;
            const float rse = interp_softmax_terms<KR>(s.low, K, s.ay, s.ax, y, s.mirror ? W - 1 - x : x, v, arg);
#pragma unroll
            for (int k = 0; k < KR; ++k) {
                if (k < K) acc[p][k] = add_rounded_product(acc[p][k], v[k], rse);
            }
            __builtin_amdgcn_sched_barrier(0);      // one pixel's loads at a time: interleaving the P pixels costs P times the registers
        }
    }
#pragma unroll
    for (int k = 0; k < KR; ++k) {
        if (k < K) {
#pragma unroll
            for (int p = 0; p < P; ++p) {
                acc[p][k] = acc[p][k] / div_a;
                if (div_b != 1.f) acc[p][k] = acc[p][k] / div_b;
            }
        }
    }
}

// The per-pixel arithmetic of the sliding-window tails (upsample_slide.hip), shared by their probability kernel and their predict-and-score
// kernel.  A source covers a rectangle of the output, not the whole of it: window i owns [y0, y0 + ay.n_out) x [x0, x0 + ax.n_out), every window
// has the same low-map and label-pixel size, hence ONE Axis pair.
struct SlideWin {
    const float* low;             // [h][w][K] logits of the window
    const float* low_mirror;      // the same of the mirrored crop (MIRROR instantiations only)
    int y0, x0;                   // origin in output coordinates
};
constexpr int MAX_SLIDE_WIN = 64;
struct SlideWins {
    SlideWin w[MAX_SLIDE_WIN];    // by value in the kernel arguments, as ProbSrcs is: no device table
};

// acc[p][k] = (q_a + q_b + ...) / cover for the P pixels (y, xb .. xb+P-1): the windows that contain the pixel, in window order from 0, with
// q_i = softmax(bilinear(low_i)) at the pixel's window-local coordinates (the device code of mi_upsample_softmax) or, with MIRROR,
// (p + pm) / 2 where pm is the same on low_mirror_i at the mirrored local column (inference(), utility.py:187-190).  Every product and sum is
// rounded on its own, the last division is a true division by the integer cover count.  cover == 1 without MIRROR: 0 + p == p and p / 1 == p,
// the bits of mi_upsample_softmax.  Nearly wave-uniform: lanes differ only at window edges; the P pixels are tested one by one (an odd x0
// puts a window edge between them).  A pixel no window covers would be 0 / 0: the launchers refuse such a grid.
template <int KR, int P, bool MIRROR>
__device__ __forceinline__ void slide_probs(const SlideWin* w_all, int n, int K, const Axis& ay, const Axis& ax, int y, int xb, float (&acc)[P][KR]) {
#pragma clang fp contract(off)
    int cover[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        cover[p] = 0;
#pragma unroll
        for (int k = 0; k < KR; ++k) acc[p][k] = 0.f;
    }
    for (int i = 0; i < n; ++i) {
        const SlideWin& s = w_all[i];
        const int yl = y - s.y0;
        if ((unsigned)yl >= (unsigned)ay.n_out) continue;
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const int xl = xb + p - s.x0;
            if ((unsigned)xl < (unsigned)ax.n_out) {
                float v[KR];
                int arg;
                const float rse = interp_softmax_terms<KR>(s.low, K, ay, ax, yl, xl, v, arg);
                if constexpr (MIRROR) {
                    float q[KR];
#pragma unroll
                    for (int k = 0; k < KR; ++k) {
                        if (k < K) q[k] = v[k] * rse;
                    }
                    const float rsm = interp_softmax_terms<KR>(s.low_mirror, K, ay, ax, yl, ax.n_out - 1 - xl, v, arg);
#pragma unroll
                    for (int k = 0; k < KR; ++k) {
                        if (k < K) {
                            const float pm = v[k] * rsm;
                            const float two = q[k] + pm;
                            acc[p][k] = acc[p][k] + two / 2.f;
                        }
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < KR; ++k) {
                        if (k < K) acc[p][k] = add_rounded_product(acc[p][k], v[k], rse);
                    }
                }
                ++cover[p];
            }
            __builtin_amdgcn_sched_barrier(0);      // one pixel's loads at a time, as in multi_probs
        }
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const float c = (float)cover[p];
#pragma unroll
        for (int k = 0; k < KR; ++k) {
            if (k < K) acc[p][k] = acc[p][k] / c;
        }
    }
}

struct ClassThr {
    float t[KMAX];               // by value in the kernel arguments, as ProbSrcs is: no device table
};

// The prediction of one pixel from its K values a[]: the LOWEST class index among their maxima (torch.max(dim) / numpy.argmax), the maximum in
// `best` and the threshold it is held against in `tb`: thr.t[0], or with CW the threshold of the WINNING class - thr.t[k] travels with the running
// maximum through the unrolled loop, so the table is read with compile-time indices (scalar registers straight from the kernel arguments), never
// with a per-lane index.  The pseudo-label is `best >= tb ? result : ignore`.
template <bool CW, int KR>
__device__ __forceinline__ int first_max(const float (&a)[KR], int K, const ClassThr& thr, float& best, float& tb) {
    best = a[0];
    tb = thr.t[0];
    int arg = 0;
#pragma unroll
    for (int k = 1; k < KR; ++k) {
        if (k < K && a[k] > best) {           // strict: the first of equal maxima stays
            best = a[k];
            arg = k;
            if constexpr (CW) tb = thr.t[k];
        }
    }
    return arg;
}

// ------------------------------------------------------------------------------------------------ the x-tile skeleton
// One workgroup per (b, y, jt_cols low-res columns): it owns the low-res columns [j0, j1) of output row y of image b; its pixels are those with x0 in
// [j0-1, j1-1], starting at xa.  Once per pixel the threads leave d[k] (the loss's derivative by the pixel's K interpolated logits) in LDS; then (j, k)
// items gather the pixels of their column support in ascending x:  tmp[b][y][j][k] = sum_x wx(x,j) d[x][k].

// The dynamic LDS of an x-tile kernel, in floats.  Each kernel has one function that returns its TileLds; the kernel takes its pointers from it
// (xtile_begin) and the launcher its byte count.
struct TileLds {
    int lam, red, pstart, vrow, extra, floats;
    __host__ __device__ TileLds(int npx_max, int K, bool with_red, int n_extra) {
        lam = npx_max * K;                          // from 0: dbuf [npx_max][K]; here: [npx_max] lambda_x
        red = lam + npx_max;                        // [512] for block_sum2, where the kernel reduces
        pstart = red + (with_red ? 512 : 0);        // [JT+3] first pixel (relative to xa) whose x0 >= j0 - 1 + q
        vrow = pstart + JT + 4;                     // [JT+2][K] low-res row already interpolated along y
        extra = vrow + (JT + 2) * K;                // [n_extra] the kernel's own
        floats = extra + n_extra;
    }
    size_t bytes() const { return (size_t)floats * sizeof(float); }
};

// tile_stage: pstart[q] = first pixel (relative to xa) whose x0 >= j0 - 1 + q, and the touched source columns (from cbase) interpolated along y into vrow.
// PINNED: the interpolation is lerp_rounded (the same bits as rowwalk_stage<true>).
template <bool PINNED = false>
__device__ __forceinline__ void tile_stage(const float* __restrict__ low, int K, const Axis& ay, const Axis& ax, int b, int y, int j0, int j1, int xa,
                                           int* pstart, float* vrow, int& cbase) {
    const int h = ay.n_in, w = ax.n_in;
    int y0, y1;
    float ly;
    ay.src(y, y0, y1, ly);
    const float* row0 = low + ((long)b * h + y0) * w * K;
    const float* row1 = low + ((long)b * h + y1) * w * K;
    cbase = max(j0 - 1, 0);
    const int ncol = min(j1, w - 1) - cbase + 1;          // source columns this tile touches
    if (threadIdx.x < j1 - j0 + 2) pstart[threadIdx.x] = ax.first_with_i0_ge(j0 - 1 + (int)threadIdx.x) - xa;
    for (int e = threadIdx.x; e < ncol * K; e += 256) {
        const long o = (long)cbase * K + e;
        if constexpr (PINNED)
            vrow[e] = lerp_rounded(ly, row0[o], row1[o]);
        else
            vrow[e] = (1.f - ly) * row0[o] + ly * row1[o];
    }
}

// tile_gather_x: trow[j][k] = sum_x wx(x,j) dbuf[x][k] for the tile's columns, (j,k) items over the threads, each in ascending x (trow: row (b, y) of tmp).
__device__ __forceinline__ void tile_gather_x(const float* dbuf, const float* lam, const int* pstart, float* __restrict__ trow, int K, int j0, int j1,
                                              int w, int npx) {
    const int nj = j1 - j0;
    for (int item = threadIdx.x; item < nj * K; item += 256) {
        const int jj = item / K, k = item - jj * K;
        const int j = j0 + jj;
        float s = 0.f;
        // pixels with x0 == j-1 contribute lam to j (as x1), then pixels with x0 == j contribute 1-lam (and lam too when x1 is
        // clamped onto j at the right edge); same weights and the same ascending-x order as a per-pixel test of x0 / x1
        const int p0 = max(pstart[jj], 0), p1 = min(max(pstart[jj + 1], 0), npx), p2 = min(pstart[jj + 2], npx);
        for (int px = p0; px < p1; ++px) s += (0.f + lam[px]) * dbuf[(long)px * K + k];
        const bool edge = j == w - 1;
        for (int px = p1; px < p2; ++px) s += ((1.f - lam[px]) + (edge ? lam[px] : 0.f)) * dbuf[(long)px * K + k];
        trow[(long)j * K + k] = s;
    }
}

// What an x-tile kernel knows about its tile after xtile_begin, and about one pixel of it after xtile_pixel.
struct XTile {
    float *dbuf, *lam, *red, *vrow, *extra;      // the LDS regions of TileLds
    int* pstart;
    int j0, j1, xa, npx, cbase;
    long row;                                    // (b * H + y): the output row, for labels (row * W + x), tmp (row * w * K) and partial (row * tiles + tile)
};
struct XPixel {
    float* d;                  // [K] the pixel's slot in dbuf
    const float *c0, *c1;      // its two staged source columns
    float lx;
    long pix;                  // index into a [B][H][W] plane
    bool own;                  // this tile accounts for the pixel (x0 >= j0; a pixel with x0 == j0-1 belongs to the previous tile)
};

// The prologue: carves the LDS, decodes the grid and stages (tile_stage).  The caller's __syncthreads() publishes the staging.
template <bool PINNED = false>
__device__ __forceinline__ XTile xtile_begin(const TileLds& L, const float* __restrict__ low, int K, const Axis& ay, const Axis& ax, int npx_max,
                                             int jt_cols) {
    extern __shared__ __attribute__((aligned(16))) float sh[];
    XTile t;
    t.dbuf = sh;
    t.lam = sh + L.lam;
    t.red = sh + L.red;
    t.pstart = reinterpret_cast<int*>(sh + L.pstart);
    t.vrow = sh + L.vrow;
    t.extra = sh + L.extra;
    const int w = ax.n_in, y = blockIdx.y, b = blockIdx.z;
    t.j0 = blockIdx.x * jt_cols;
    t.j1 = min(w, t.j0 + jt_cols);
    t.xa = ax.first_with_i0_ge(t.j0 - 1);                                   // pixels with x0 in [j0-1, j1-1]
    t.npx = min(ax.first_with_i0_ge(t.j1) - t.xa, npx_max);
    t.row = (long)b * ay.n_out + y;
    tile_stage<PINNED>(low, K, ay, ax, b, y, t.j0, t.j1, t.xa, t.pstart, t.vrow, t.cbase);
    return t;
}

// Pixel px of the tile (the loop is `for (int px = threadIdx.x; px < t.npx; px += 256)`): stores its lambda_x for the gather.
__device__ __forceinline__ XPixel xtile_pixel(const XTile& t, const Axis& ax, int K, int px) {
    const int x = t.xa + px;
    int x0, x1;
    XPixel q;
    ax.src(x, x0, x1, q.lx);
    t.lam[px] = q.lx;
    q.d = t.dbuf + (long)px * K;
    q.c0 = t.vrow + (x0 - t.cbase) * K;
    q.c1 = t.vrow + (x1 - t.cbase) * K;
    q.pix = t.row * ax.n_out + x;
    q.own = x0 >= t.j0;
    return q;
}

// The epilogue, after the __syncthreads() that publishes dbuf: the gather into row (b, y) of tmp.
__device__ __forceinline__ void xtile_gather(const XTile& t, float* __restrict__ tmp, int K, int w) {
    tile_gather_x(t.dbuf, t.lam, t.pstart, tmp + t.row * w * K, K, t.j0, t.j1, w, t.npx);
}

// ------------------------------------------------------------------------------------------------ the row-walk skeleton
// One workgroup per (b, `rows` output rows, GDL_XT output columns); a thread keeps one column and walks the rows, what it accumulates in registers:
//   const RowWalk r = rowwalk_begin(ay, ax, rows, ncol_max);
//   for (int y = r.ya; y < r.yb; ++y) {
//       rowwalk_stage(r, low, vrow, K, ay, ax.n_in, y);      // the row's touched source columns interpolated along y into vrow ([ncol_max][K]), and a barrier
//       if (r.live) { ... the pixel r.pix(ay, ax, y) from vrow + r.c0 * K and vrow + r.c1 * K with r.lx ... }
//       __syncthreads();                                     // the next row overwrites vrow
//   }
// The epilogues (how a workgroup reduces what its threads hold) differ and stay with the kernels.
struct RowWalk {
    int b, ya, yb, x, cbase, ncol, c0, c1;      // c0, c1: the thread's two source columns relative to cbase
    float lx;
    bool live;                                  // the thread has a column (x < xb)
    __device__ __forceinline__ long pix(const Axis& ay, const Axis& ax, int y) const { return ((long)b * ay.n_out + y) * ax.n_out + x; }
};

__device__ __forceinline__ RowWalk rowwalk_begin(const Axis& ay, const Axis& ax, int rows, int ncol_max) {
    RowWalk r;
    const int H = ay.n_out, W = ax.n_out;
    r.b = blockIdx.z;
    const int xa = blockIdx.x * GDL_XT, xb = min(W, xa + GDL_XT);
    r.ya = blockIdx.y * rows;
    r.yb = min(H, r.ya + rows);
    int clast, unused;
    r.lx = 0.f;
    ax.src(xa, r.cbase, unused, r.lx);
    ax.src(xb - 1, unused, clast, r.lx);
    r.ncol = min(clast - r.cbase + 1, ncol_max);      // upsampling: x0 advances by at most one per pixel, so GDL_XT pixels touch at most GDL_XT + 1 columns
    r.x = xa + threadIdx.x;
    r.live = r.x < xb;
    int x0 = r.cbase, x1 = r.cbase;
    if (r.live) ax.src(r.x, x0, x1, r.lx);
    r.c0 = x0 - r.cbase;
    r.c1 = x1 - r.cbase;
    return r;
}

template <bool PINNED = false>
__device__ __forceinline__ void rowwalk_stage(const RowWalk& r, const float* __restrict__ low, float* vrow, int K, const Axis& ay, int w, int y) {
    int y0, y1;
    float ly;
    ay.src(y, y0, y1, ly);
    const float* row0 = low + (((long)r.b * ay.n_in + y0) * w + r.cbase) * K;
    const float* row1 = low + (((long)r.b * ay.n_in + y1) * w + r.cbase) * K;
    for (int e = threadIdx.x; e < r.ncol * K; e += 256) {
        if constexpr (PINNED)
            vrow[e] = lerp_rounded(ly, row0[e], row1[e]);
        else
            vrow[e] = (1.f - ly) * row0[e] + ly * row1[e];
    }
    __syncthreads();
}

// pass 2: dlow[b][i][j][k] = grad_scale / n_valid * sum_y wy(y,i) tmp[b][y][j][k]   (ascending y)
// ZERO_STAYS: a sum that is exactly 0 stays 0 whatever the divisor (torch leaves the gradient of ignored pixels at 0 when no pixel counts, S = 0;
// 0 * (grad_scale / 0) would be nan).  Any other sum is scaled as before.
template <bool ZERO_STAYS>
__device__ __forceinline__ void pass2_body(const float* __restrict__ tmp, const float* __restrict__ loss_out, float* __restrict__ dlow, int B, int K,
                                           const Axis& ay, int w, float grad_scale) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int H = ay.n_out, h = ay.n_in;
    const long per_row = (long)w * K;
    if (idx >= (long)B * h * per_row) return;
    const long jk = idx % per_row;
    const int i = (int)((idx / per_row) % h), b = (int)(idx / (per_row * h));
    const int ya = ay.first_with_i0_ge(i - 1), yb = ay.first_with_i0_ge(i + 1);
    float s = 0.f;
    for (int y = ya; y < yb; ++y) {
        int y0, y1;
        float ly;
        ay.src(y, y0, y1, ly);
        const float wy = (y0 == i ? 1.f - ly : 0.f) + (y1 == i ? ly : 0.f);
        s += wy * tmp[((long)b * H + y) * per_row + jk];
    }
    const float r = s * (loss_out ? grad_scale / loss_out[1] : grad_scale);      // (no loss_out: the Dice gradient, whose coefficients carry its normalisation)
    dlow[idx] = (ZERO_STAYS && s == 0.f) ? 0.f : r;
}

// ------------------------------------------------------------------------------------------------ launch planning
inline unsigned nblk(long n, int bs) { return (unsigned)((n + bs - 1) / bs); }
inline size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

inline int pass1_npx_max(const Axis& ax, int jt_cols) {
    // upper bound of pixels whose x0 falls in jt_cols+1 consecutive source columns
    if (ax.scale <= 0.f) return ax.n_out;
    const long n = (long)((float)(jt_cols + 1) / ax.scale) + 4;
    return (int)(n < ax.n_out ? n : ax.n_out);
}

// Low-res columns per workgroup: 32 up to an 8x upsample, fewer above (a tile of 32 columns at 32x is 1 056 pixels x 19 classes = 80 KB of LDS: one
// workgroup per CU - the 1/32 head of GALD took 788 us against 204 us for the 1/4 head with the same 5.5 M pixels); about 256 pixels per tile.
inline int pick_jt(int w, int W) {
    const int f = w > 0 ? (W + w - 1) / w : 1;
    int jt = JT;
    while (jt > 4 && jt * f > 256) jt >>= 1;
    return jt;
}

// The row-walk grid: GDL_XT-column tiles, and as many rows per workgroup as keep the launch near 1024 workgroups (4 per CU, what the Dice reduction's
// registers let a CU hold: one round; and the partial rows a one-workgroup finalize has to add stay a few hundred KB at 6 x 720 x 1280).
struct GdlPlan {
    int tiles_x, rows, row_groups;
    size_t nwg;
};
inline GdlPlan gdl_plan(int B, int H, int W) {
    GdlPlan p;
    p.tiles_x = (W + GDL_XT - 1) / GDL_XT;
    const long units = (long)B * H * p.tiles_x;
    long rows = (units + 1023) / 1024;
    p.rows = (int)(rows < 1 ? 1 : (rows > H ? H : rows));
    p.row_groups = (H + p.rows - 1) / p.rows;
    p.nwg = (size_t)B * p.row_groups * p.tiles_x;
    return p;
}

// f(std::integral_constant<int, KT>) with KT = 19 when K is 19, else 0 (K read at run time): the two instantiations every K-templated kernel has.
template <class F>
inline void with_kt(int K, F&& f) {
    if (K == 19)
        f(std::integral_constant<int, 19>{});
    else
        f(std::integral_constant<int, 0>{});
}

// ------------------------------------------------------------------------------------------------ launch helpers of the fused heads (upsample_ce.hip, upsample_lovasz.hip)
// What every fused head requires of its shapes; `who` names the entry that was called, ktext what its K may be.
inline int head_check(const char* who, int B, int h, int w, int K, int H, int W, const char* ktext = " (K <= 32)") {
    MI_REQUIRE(B > 0 && h > 0 && w > 0 && H > 0 && W > 0 && K > 0 && K <= KMAX, "%s: bad dimension%s", who, ktext);
    MI_REQUIRE(H >= h && W >= w, "%s: only upsampling (H >= h, W >= w) is supported", who);
    MI_REQUIRE(H <= 65535 && B <= 65535, "%s: grid dimension overflow", who);
    return MI_OK;
}

struct HeadPlan {          // the two axes and the x-tile grid
    Axis ay, ax;
    int jt_cols, tiles, npx_max;
};
inline HeadPlan head_plan(int h, int w, int H, int W, int align_corners) {
    HeadPlan p;
    p.ay = make_axis(h, H, align_corners);
    p.ax = make_axis(w, W, align_corners);
    p.jt_cols = pick_jt(w, W);
    p.tiles = (w + p.jt_cols - 1) / p.jt_cols;
    p.npx_max = pass1_npx_max(p.ax, p.jt_cols);
    return p;
}

// Launch of an x-tile kernel.  Its LDS varies with the upsample factor: the maximum is allowed once per (kernel, device).
template <auto Kern, class... Args>
void launch_xtile(const HeadPlan& p, int H, int B, size_t lds, hipStream_t st, Args... args) {
    static std::atomic<uint64_t> lds_set;
    mi_allow_dynamic_lds((const void*)Kern, MI_LDS_MAX, lds_set);
    hipLaunchKernelGGL(Kern, dim3(p.tiles, H, B), dim3(256), lds, st, args...);
}

inline int launch_failed(const char* who, const char* step) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MI_OK : mi_set_error(MI_EHIP, "%s %s: %s", who, step, hipGetErrorString(e));
}

}  // namespace
