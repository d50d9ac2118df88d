// Bilinear upsample (align_corners=True), per-pixel softmax cross-entropy with ignore_index, and their fusion.
//   F.interpolate(..., mode='bilinear', align_corners=True)   reference core/models/classifiers/aspp/classifier.py:31,
//                                                              core/utils/utility.py:185
//   torch.nn.CrossEntropyLoss(ignore_index=255)               reference core/trainers/aspp_trainer.py:61,91
//   softmax over classes for inference                        reference core/utils/utility.py:186
// All arithmetic fp32 (kept fp32 in bf16 mode too).  HBM-bound: the fused training path reads the
// 1/8-resolution logits (5.7 MB at B=8, 769x769) and labels and never writes the 360 MB [B,19,769,769] tensor.
// Every reduction has a fixed summation order (no float atomics) so results are bitwise reproducible.
#include "mi_common.h"
#include <cmath>

namespace {

constexpr int KMAX = 32;   // classes held in registers

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

__device__ __forceinline__ float lerp2(float v00, float v01, float v10, float v11, float lx, float ly) {
    return (1.f - ly) * ((1.f - lx) * v00 + lx * v01) + ly * ((1.f - lx) * v10 + lx * v11);
}

// ------------------------------------------------------------------------------------------------ unfused
__global__ void upsample_fwd_kernel(const float* __restrict__ low, float* __restrict__ up, int B, int K, Axis ay, Axis ax) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int H = ay.n_out, W = ax.n_out, h = ay.n_in, w = ax.n_in;
    if (idx >= (long)B * H * W) return;
    const int x = (int)(idx % W), y = (int)((idx / W) % H), b = (int)(idx / ((long)W * H));
    int y0, y1, x0, x1;
    float ly, lx;
    ay.src(y, y0, y1, ly);
    ax.src(x, x0, x1, lx);
    const float* p00 = low + (((long)b * h + y0) * w + x0) * K;
    const float* p01 = low + (((long)b * h + y0) * w + x1) * K;
    const float* p10 = low + (((long)b * h + y1) * w + x0) * K;
    const float* p11 = low + (((long)b * h + y1) * w + x1) * K;
    float* o = up + ((long)b * K * H + y) * W + x;
    for (int k = 0; k < K; ++k) o[(long)k * H * W] = lerp2(p00[k], p01[k], p10[k], p11[k], lx, ly);
}

// gather form: thread per (b,k,i,j), j fastest; sums contributions in (y,x) ascending order
__global__ void upsample_bwd_kernel(const float* __restrict__ dup, float* __restrict__ dlow, int B, int K, Axis ay, Axis ax) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int H = ay.n_out, W = ax.n_out, h = ay.n_in, w = ax.n_in;
    if (idx >= (long)B * K * h * w) return;
    const int j = (int)(idx % w), i = (int)((idx / w) % h), k = (int)((idx / ((long)w * h)) % K), b = (int)(idx / ((long)w * h * K));
    const int ya = ay.first_with_i0_ge(i - 1), yb = ay.first_with_i0_ge(i + 1);
    const int xa = ax.first_with_i0_ge(j - 1), xb = ax.first_with_i0_ge(j + 1);
    const float* src = dup + ((long)b * K + k) * H * W;
    float s = 0.f;
    for (int y = ya; y < yb; ++y) {
        int y0, y1;
        float ly;
        ay.src(y, y0, y1, ly);
        const float wy = (y0 == i ? 1.f - ly : 0.f) + (y1 == i ? ly : 0.f);
        if (wy == 0.f && y0 != i && y1 != i) continue;
        float r = 0.f;
        for (int x = xa; x < xb; ++x) {
            int x0, x1;
            float lx;
            ax.src(x, x0, x1, lx);
            const float wx = (x0 == j ? 1.f - lx : 0.f) + (x1 == j ? lx : 0.f);
            r += wx * src[(long)y * W + x];
        }
        s += wy * r;
    }
    dlow[(((long)b * h + i) * w + j) * K + k] = s;
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

// Labels outside [0, K) that are not ignore_index: torch.nn.CrossEntropyLoss raises a device assert; here they are excluded
// from the loss AND counted (integer atomic: order-independent) so that the host can refuse the batch (loss_out[2]).
__device__ __forceinline__ void count_bad_label(long lab, int K, int ignore_index, unsigned* bad) {
    if (lab != ignore_index && (lab < 0 || lab >= K)) atomicAdd(bad, 1u);
}

__global__ void ce_fwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels, float* __restrict__ partial,
                              int B, int K, long HW, int ignore_index, unsigned* __restrict__ bad) {
    __shared__ float red[512];
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    float loss = 0.f, cnt = 0.f;
    if (idx < (long)B * HW) {
        const long b = idx / HW, pix = idx - b * HW;
        const long lab = labels[idx];
        count_bad_label(lab, K, ignore_index, bad);
        if (lab != ignore_index && lab >= 0 && lab < K) {
            const float* p = logits + b * K * HW + pix;
            float mx = p[0];
            for (int k = 1; k < K; ++k) mx = fmaxf(mx, p[k * HW]);
            float se = 0.f;
            for (int k = 0; k < K; ++k) se += __expf(p[k * HW] - mx);
            loss = (mx + __logf(se)) - p[lab * HW];
            cnt = 1.f;
        }
    }
    block_sum2(loss, cnt, red);
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = loss;
        partial[2 * blockIdx.x + 1] = cnt;
    }
}

__global__ void ce_finalize_kernel(const float* __restrict__ partial, int n, float* __restrict__ loss_out) {
    __shared__ float red[512];
    float s = 0.f, c = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
        s += partial[2 * i];
        c += partial[2 * i + 1];
    }
    block_sum2(s, c, red);
    if (threadIdx.x == 0) {
        loss_out[0] = s / c;   // 0/0 = nan when every pixel is ignored, like torch
        loss_out[1] = c;
        loss_out[2] = (float)*reinterpret_cast<const unsigned*>(loss_out + 3);      // out-of-range labels seen by pass 1
    }
}

__global__ void ce_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels, const float* __restrict__ loss_out,
                              float* __restrict__ dlogits, int B, int K, long HW, int ignore_index, float grad_scale) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)B * HW) return;
    const long b = idx / HW, pix = idx - b * HW;
    const long lab = labels[idx];
    const float* p = logits + b * K * HW + pix;
    float* d = dlogits + b * K * HW + pix;
    if (lab == ignore_index || lab < 0 || lab >= K) {
        for (int k = 0; k < K; ++k) d[k * HW] = 0.f;
        return;
    }
    const float inv = grad_scale / loss_out[1];
    float mx = p[0];
    for (int k = 1; k < K; ++k) mx = fmaxf(mx, p[k * HW]);
    float se = 0.f;
    for (int k = 0; k < K; ++k) se += __expf(p[k * HW] - mx);
    const float rse = 1.f / se;
    for (int k = 0; k < K; ++k) d[k * HW] = (__expf(p[k * HW] - mx) * rse - (k == lab ? 1.f : 0.f)) * inv;
}

// ------------------------------------------------------------------------------------------------ fused
// pass 1: one workgroup per (b, y, tile of JT low-res columns).  Threads compute, ONCE per high-res pixel, the
// interpolated logits, the loss term and d = softmax - onehot into LDS; then (j,k) items gather the pixels of
// their column support in ascending x:  tmp[b][y][j][k] = sum_x wx(x,j) d[x][k].
constexpr int JT = 32;              // the largest tile; the launcher narrows it for large upsample factors (pick_jt)

// What the x-tile kernels (upce_pass1_kernel, gdl_grad_kernel) share.  A workgroup owns the low-res columns [j0, j1) of output row y of image b:
// its pixels are those with x0 in [j0-1, j1-1], starting at xa.
// tile_stage: pstart[q] = first pixel (relative to xa) whose x0 >= j0 - 1 + q, and the touched source columns (from cbase) interpolated along y into vrow.
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

// KT > 0: the class count is a compile-time constant (19 for Cityscapes: exact-length register loops instead of 32 predicated
// iterations); KT == 0: K is read from the arguments.
// MODE == UPCE_WEIGHTED (mi_upsample_ce_w): torch's CrossEntropyLoss(weight=, label_smoothing=s).  Per valid pixel, with lp_c = (z_c - max) - log(sum exp):
//   loss term = (1-s) w_y (-lp_y) + s/K sum_c w_c (-lp_c),  d_k = (1-s) w_y (p_k - [k==y]) + s/K (p_k Wsum - w_k),  "count" = w_y  (so that the
// finalize divides by S = sum_valid w_y and pass 2 by loss_out[1] as ever).  wce.cw (NULL: all 1) is read from device memory by every workgroup into
// LDS - K floats, a label-indexed ds_read per pixel instead of a global load - with Wsum behind them, added in class order.
// MODE == UPCE_PLAIN compiles none of it: wce is an unused kernel argument.
enum { UPCE_PLAIN = 0, UPCE_WEIGHTED = 1 };
struct WceArgs {
    const float* cw;      // [K] class weights on the device, or NULL
    float keep;           // 1 - s
    float smooth;         // s / K
};

template <int KT, int MODE = UPCE_PLAIN>
__global__ __launch_bounds__(256) void upce_pass1_kernel(const float* __restrict__ low, const int64_t* __restrict__ labels,
                                                         float* __restrict__ partial, float* __restrict__ tmp, int B, int Krt, Axis ay,
                                                         Axis ax, int ignore_index, int npx_max, unsigned* __restrict__ bad, int jt_cols, WceArgs wce) {
    const int K = KT > 0 ? KT : Krt;
    constexpr int KR = KT > 0 ? KT : KMAX;          // register array length
    extern __shared__ __attribute__((aligned(16))) float sh[];
    float* dbuf = sh;                               // [npx_max][K]
    float* lam = sh + (long)npx_max * K;            // [npx_max]  lambda_x
    int* x0s = reinterpret_cast<int*>(lam + npx_max);  // [npx_max]  x0
    float* red = reinterpret_cast<float*>(x0s + npx_max);  // [512]
    int* pstart = reinterpret_cast<int*>(red + 512);   // [JT+3] first pixel (relative to xa) whose x0 >= j0 - 1 + q
    float* vrow = red + 512 + JT + 4;                // [JT+2][K] low-res row already interpolated along y
    const int H = ay.n_out, W = ax.n_out, h = ay.n_in, w = ax.n_in;
    const int jt = blockIdx.x, y = blockIdx.y, b = blockIdx.z;
    const int j0 = jt * jt_cols, j1 = min(w, j0 + jt_cols);
    const int xa = ax.first_with_i0_ge(j0 - 1), xb = ax.first_with_i0_ge(j1);   // pixels with x0 in [j0-1, j1-1]
    const int npx = xb - xa;
    int cbase;
    tile_stage(low, K, ay, ax, b, y, j0, j1, xa, pstart, vrow, cbase);
    float* wsh = vrow + (JT + 2) * K;               // UPCE_WEIGHTED: [K] class weights, then Wsum
    if constexpr (MODE == UPCE_WEIGHTED) {
        if (threadIdx.x < K) wsh[threadIdx.x] = wce.cw ? wce.cw[threadIdx.x] : 1.f;
        __syncthreads();
        if (threadIdx.x == 0) {
            float t = 0.f;
            for (int k = 0; k < K; ++k) t += wsh[k];
            wsh[K] = t;
        }
    }
    __syncthreads();
    float loss = 0.f, cnt = 0.f;
    for (int px = threadIdx.x; px < npx; px += 256) {
        const int x = xa + px;
        int x0, x1;
        float lx;
        ax.src(x, x0, x1, lx);
        lam[px] = lx;
        const long lab = labels[((long)b * H + y) * W + x];
        float* d = dbuf + (long)px * K;
        if (x0 >= j0) count_bad_label(lab, K, ignore_index, bad);       // once per pixel: by the tile that owns it
        if (lab == ignore_index || lab < 0 || lab >= K) {
            for (int k = 0; k < K; ++k) d[k] = 0.f;
            continue;
        }
        const float* c0 = vrow + (x0 - cbase) * K;
        const float* c1 = vrow + (x1 - cbase) * K;
        float v[KR];
        float mx = -3.0e38f;
#pragma unroll
        for (int k = 0; k < KR; ++k) {
            if (k < K) {
                v[k] = (1.f - lx) * c0[k] + lx * c1[k];
                mx = fmaxf(mx, v[k]);
            }
        }
        float se = 0.f, picked = 0.f;          // picked = x[label] - max BEFORE the exponential: exp() of it underflows to 0 for
        float wz = 0.f;                        // a confidently wrong pixel (|logit| gap > 87) and log(0) would make the loss inf
#pragma unroll                                // wz (UPCE_WEIGHTED) = sum_c w_c (z_c - max), before the exponential for the same reason
        for (int k = 0; k < KR; ++k) {
            if (k < K) {
                if (k == lab) picked = v[k] - mx;
                if constexpr (MODE == UPCE_WEIGHTED) wz += wsh[k] * (v[k] - mx);
                v[k] = __expf(v[k] - mx);
                se += v[k];
            }
        }
        const float rse = 1.f / se;
        if constexpr (MODE == UPCE_WEIGHTED) {
            const float wy = wsh[lab], wsum = wsh[K];
            const float hard = wce.keep * wy;
#pragma unroll
            for (int k = 0; k < KR; ++k) {
                if (k < K) {
                    const float t = v[k] * rse - (k == lab ? 1.f : 0.f);
                    d[k] = hard * t + wce.smooth * ((v[k] * rse) * wsum - wsh[k]);
                }
            }
            if (x0 >= j0) {
                const float lse = __logf(se);
                const float nll = lse - picked;
                loss += hard * nll + wce.smooth * (wsum * lse - wz);          // sum_c w_c (-lp_c) = Wsum lse - sum_c w_c (z_c - max)
                cnt += wy;
            }
            continue;
        }
#pragma unroll
        for (int k = 0; k < KR; ++k) {
            if (k < K) d[k] = v[k] * rse - (k == lab ? 1.f : 0.f);
        }
        if (x0 >= j0) {   // the tile that owns x0 accounts for the loss (x0 == j0-1 pixels belong to the previous tile)
            loss += __logf(se) - picked;          // = logsumexp(x) - x[label], like ATen's log_softmax + nll_loss
            cnt += 1.f;
        }
    }
    __syncthreads();
    if (tmp) tile_gather_x(dbuf, lam, pstart, tmp + ((long)b * H + y) * w * K, K, j0, j1, w, npx);
    block_sum2(loss, cnt, red);
    if (threadIdx.x == 0) {
        const long pidx = ((long)b * H + y) * gridDim.x + jt;
        partial[2 * pidx] = loss;
        partial[2 * pidx + 1] = cnt;
    }
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

__global__ void upce_pass2_kernel(const float* __restrict__ tmp, const float* __restrict__ loss_out, float* __restrict__ dlow, int B, int K,
                                  Axis ay, int w, float grad_scale) {
    pass2_body<false>(tmp, loss_out, dlow, B, K, ay, w, grad_scale);
}

__global__ void wce_pass2_kernel(const float* __restrict__ tmp, const float* __restrict__ loss_out, float* __restrict__ dlow, int B, int K,
                                 Axis ay, int w, float grad_scale) {
    pass2_body<true>(tmp, loss_out, dlow, B, K, ay, w, grad_scale);
}

// ------------------------------------------------------------------------------------------------ generalized Dice, fused with the upsample
// GeneralizedDiceLoss (reference core/utils/utility.py:399-447, label form) on z = bilinear(low), m = (label != ignore_index):
//   p = softmax_k(z) m, t = onehot(label) m;  T_c = sum t, I_c = sum p t, P2_c = sum p^2;  w_c = 1 / (T_c^2 + eps) | 1 / (T_c + eps) | 1 / (sqrt(T_c) + eps)
//   Num = sum_c w_c I_c, Den = sum_c w_c (P2_c + T_c) + eps, loss = 1 - 2 Num / Den
//   d loss / d z_k = p_k (g_k - sum_j g_j p_j) on valid pixels, g_c = a_c t_c + b_c p_c, a_c = -2 w_c / Den, b_c = 4 Num w_c / Den^2
// The coefficients depend on sums over the whole batch, so the gradient is a second pass that recomputes the softmax from `low`:
//   gdl_reduce_kernel (per-workgroup partial T / I / P2) -> gdl_finalize_kernel (one workgroup: loss, a_c, b_c in device memory) ->
//   gdl_grad_kernel (d loss / d z gathered along x, the skeleton of upce_pass1_kernel) -> upce_pass2_kernel (gathered along y).
// Fixed summation order everywhere; T_c and the bad-label count are integers.
constexpr int GDL_XT = 256;          // output pixels of one row per workgroup in the reduction pass: one per thread and row

__device__ __forceinline__ float wave_sum(float v) {          // xor butterfly: both partners add the same two values, every lane ends with the same bits
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ unsigned wave_sum(unsigned v) {
    for (int m = 32; m > 0; m >>= 1) v += (unsigned)__shfl_xor((int)v, m);
    return v;
}

// One workgroup per (b, `rows` output rows, GDL_XT output columns); a thread keeps one column and walks the rows with its 3K sums in registers.
// partial: [workgroup][3K + 1] 32-bit words - T_c (unsigned), the bad-label count (unsigned), I_c (float), P2_c (float).
template <int KT>
__global__ __launch_bounds__(256) void gdl_reduce_kernel(const float* __restrict__ low, const int64_t* __restrict__ labels, unsigned* __restrict__ partial,
                                                         int Krt, Axis ay, Axis ax, int ignore_index, int rows, int ncol_max) {
    const int K = KT > 0 ? KT : Krt;
    constexpr int KR = KT > 0 ? KT : KMAX;
    extern __shared__ __attribute__((aligned(16))) float sh[];
    float* vrow = sh;                                                          // [ncol_max][K] source row already interpolated along y
    unsigned* red = reinterpret_cast<unsigned*>(sh + (long)ncol_max * K);      // [4][3K + 1]
    const int H = ay.n_out, W = ax.n_out, h = ay.n_in, w = ax.n_in;
    const int NC = 3 * K + 1, tid = threadIdx.x, b = blockIdx.z;
    const int xa = blockIdx.x * GDL_XT, xb = min(W, xa + GDL_XT);
    const int ya = blockIdx.y * rows, yb = min(H, ya + rows);
    int cbase, clast, unused;
    float lx = 0.f;
    ax.src(xa, cbase, unused, lx);
    ax.src(xb - 1, unused, clast, lx);
    const int ncol = min(clast - cbase + 1, ncol_max);      // upsampling: x0 advances by at most one per pixel, so GDL_XT pixels touch at most GDL_XT + 1 columns
    const int x = xa + tid;
    int x0 = cbase, x1 = cbase;
    if (x < xb) ax.src(x, x0, x1, lx);
    float p2[KR], it[KR];
    unsigned tc[KR], bad = 0u;
#pragma unroll
    for (int k = 0; k < KR; ++k) {
        p2[k] = 0.f;
        it[k] = 0.f;
        tc[k] = 0u;
    }
    for (int y = ya; y < yb; ++y) {
        int y0, y1;
        float ly;
        ay.src(y, y0, y1, ly);
        const float* row0 = low + (((long)b * h + y0) * w + cbase) * K;
        const float* row1 = low + (((long)b * h + y1) * w + cbase) * K;
        for (int e = tid; e < ncol * K; e += 256) vrow[e] = (1.f - ly) * row0[e] + ly * row1[e];
        __syncthreads();
        if (x < xb) {
            const long lab = labels[((long)b * H + y) * W + x];
            if (lab != ignore_index && lab >= 0 && lab < K) {
                const float* c0 = vrow + (x0 - cbase) * K;
                const float* c1 = vrow + (x1 - cbase) * K;
                float v[KR];
                float mx = -3.0e38f;
#pragma unroll
                for (int k = 0; k < KR; ++k) {
                    if (k < K) {
                        v[k] = (1.f - lx) * c0[k] + lx * c1[k];
                        mx = fmaxf(mx, v[k]);
                    }
                }
                float se = 0.f;
#pragma unroll
                for (int k = 0; k < KR; ++k) {
                    if (k < K) {
                        v[k] = __expf(v[k] - mx);
                        se += v[k];
                    }
                }
                const float rse = 1.f / se;
#pragma unroll
                for (int k = 0; k < KR; ++k) {
                    if (k < K) {
                        const float p = v[k] * rse;
                        p2[k] += p * p;
                        if (k == lab) {
                            it[k] += p;
                            tc[k] += 1u;
                        }
                    }
                }
            } else if (lab != ignore_index) {
                bad += 1u;
            }
        }
        __syncthreads();          // the next row overwrites vrow
    }
    const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int k = 0; k < KR; ++k) {
        if (k < K) {
            const unsigned t = wave_sum(tc[k]);
            const float a = wave_sum(it[k]), q = wave_sum(p2[k]);
            if (lane == 0) {
                red[wv * NC + k] = t;
                red[wv * NC + K + 1 + k] = __float_as_uint(a);
                red[wv * NC + 2 * K + 1 + k] = __float_as_uint(q);
            }
        }
    }
    bad = wave_sum(bad);
    if (lane == 0) red[wv * NC + K] = bad;
    __syncthreads();
    if (tid < NC) {
        const long wg = ((long)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        unsigned r;
        if (tid <= K)
            r = red[tid] + red[NC + tid] + red[2 * NC + tid] + red[3 * NC + tid];
        else
            r = __float_as_uint(((__uint_as_float(red[tid]) + __uint_as_float(red[NC + tid])) + __uint_as_float(red[2 * NC + tid])) +
                                __uint_as_float(red[3 * NC + tid]));
        partial[wg * NC + tid] = r;
    }
}

__device__ __forceinline__ double gdl_weight(double T, int weight_type, double eps) {
    return 1.0 / ((weight_type == 0 ? T * T : weight_type == 1 ? T : sqrt(T)) + eps);
}

// One workgroup of GDL_FIN_WAVES waves: the partial rows summed in a fixed order (wave w takes rows w, w + 16, ... with four loads in flight; integers in
// 64 bits, floats in fp64), then the loss and the 2K gradient coefficients.  loss_out: loss, valid pixels, bad labels, 0.  sums (nullable): [3K] T, I, P2.
// The loop is a chain of memory round trips, hence 16 waves with four loads in flight each: 16 us for the 990 rows of a 6 x 720 x 1280 head.
constexpr int GDL_FIN_WAVES = 16;
__global__ __launch_bounds__(64 * GDL_FIN_WAVES) void gdl_finalize_kernel(const unsigned* __restrict__ partial, int n, int K, int weight_type, float eps,
                                                                          float* __restrict__ loss_out, float* __restrict__ coef, float* __restrict__ sums) {
    __shared__ double red[GDL_FIN_WAVES][3 * KMAX + 1];
    __shared__ double tot[3 * KMAX + 1];
    __shared__ double nd[2];
    const int NC = 3 * K + 1, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    constexpr int S = GDL_FIN_WAVES;
    for (int c = lane; c < NC; c += 64) {
        const unsigned* col = partial + c;
        double s = 0.0;
        int i = wv;
        if (c <= K) {
            unsigned long long u = 0ull;
            for (; i + 3 * S < n; i += 4 * S)
                u += ((unsigned long long)col[(long)i * NC] + col[(long)(i + S) * NC]) + ((unsigned long long)col[(long)(i + 2 * S) * NC] + col[(long)(i + 3 * S) * NC]);
            for (; i < n; i += S) u += col[(long)i * NC];
            s = (double)u;
        } else {
            for (; i + 3 * S < n; i += 4 * S)
                s += ((double)__uint_as_float(col[(long)i * NC]) + (double)__uint_as_float(col[(long)(i + S) * NC])) +
                     ((double)__uint_as_float(col[(long)(i + 2 * S) * NC]) + (double)__uint_as_float(col[(long)(i + 3 * S) * NC]));
            for (; i < n; i += S) s += (double)__uint_as_float(col[(long)i * NC]);
        }
        red[wv][c] = s;
    }
    __syncthreads();
    if (tid < NC) {
        double s = 0.0;
        for (int w = 0; w < S; ++w) s += red[w][tid];
        tot[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        double num = 0.0, den = 0.0, valid = 0.0;
        for (int c = 0; c < K; ++c) {
            const double T = tot[c], wc = gdl_weight(T, weight_type, (double)eps);
            num += wc * tot[K + 1 + c];
            den += wc * (tot[2 * K + 1 + c] + T);
            valid += T;
        }
        den += (double)eps;
        nd[0] = num;
        nd[1] = den;
        loss_out[0] = (float)(1.0 - 2.0 * num / den);      // every pixel ignored: num = 0, den = eps, the loss is exactly 1
        loss_out[1] = (float)valid;
        loss_out[2] = (float)tot[K];
        loss_out[3] = 0.f;
    }
    __syncthreads();
    if (tid < K) {
        const double num = nd[0], den = nd[1], wc = gdl_weight(tot[tid], weight_type, (double)eps);
        coef[tid] = (float)(-2.0 * wc / den);
        coef[K + tid] = (float)(4.0 * num * wc / (den * den));
        if (sums) {
            sums[tid] = (float)tot[tid];
            sums[K + tid] = (float)tot[K + 1 + tid];
            sums[2 * K + tid] = (float)tot[2 * K + 1 + tid];
        }
    }
}

// The tiling of upce_pass1_kernel (one workgroup per (b, y, jt_cols low-res columns), pixels of the tile's column support in LDS, gathered per (j, k) in
// ascending x: tile_stage / tile_gather_x) with d = d loss / d z of the Dice loss from the coefficients the finalize left in `coef` ([K] a_c, [K] b_c).
template <int KT>
__global__ __launch_bounds__(256) void gdl_grad_kernel(const float* __restrict__ low, const int64_t* __restrict__ labels, const float* __restrict__ coef,
                                                       float* __restrict__ tmp, int Krt, Axis ay, Axis ax, int ignore_index, int npx_max, int jt_cols) {
    const int K = KT > 0 ? KT : Krt;
    constexpr int KR = KT > 0 ? KT : KMAX;
    extern __shared__ __attribute__((aligned(16))) float sh[];
    float* dbuf = sh;                                           // [npx_max][K]
    float* lam = sh + (long)npx_max * K;                        // [npx_max]  lambda_x
    int* pstart = reinterpret_cast<int*>(lam + npx_max);        // [JT+3] first pixel (relative to xa) whose x0 >= j0 - 1 + q
    float* vrow = reinterpret_cast<float*>(pstart + JT + 4);    // [JT+2][K] low-res row already interpolated along y
    const int H = ay.n_out, W = ax.n_out, h = ay.n_in, w = ax.n_in;
    const int jt = blockIdx.x, y = blockIdx.y, b = blockIdx.z;
    const int j0 = jt * jt_cols, j1 = min(w, j0 + jt_cols);
    const int xa = ax.first_with_i0_ge(j0 - 1), xb = ax.first_with_i0_ge(j1);   // pixels with x0 in [j0-1, j1-1]
    const int npx = min(xb - xa, npx_max);
    int cbase;
    tile_stage(low, K, ay, ax, b, y, j0, j1, xa, pstart, vrow, cbase);
    __syncthreads();
    for (int px = threadIdx.x; px < npx; px += 256) {
        const int x = xa + px;
        int x0, x1;
        float lx;
        ax.src(x, x0, x1, lx);
        lam[px] = lx;
        const long lab = labels[((long)b * H + y) * W + x];
        float* d = dbuf + (long)px * K;
        if (lab == ignore_index || lab < 0 || lab >= K) {
            for (int k = 0; k < K; ++k) d[k] = 0.f;
            continue;
        }
        const float* c0 = vrow + (x0 - cbase) * K;
        const float* c1 = vrow + (x1 - cbase) * K;
        float v[KR];
        float mx = -3.0e38f;
#pragma unroll
        for (int k = 0; k < KR; ++k) {
            if (k < K) {
                v[k] = (1.f - lx) * c0[k] + lx * c1[k];
                mx = fmaxf(mx, v[k]);
            }
        }
        float se = 0.f;
#pragma unroll
        for (int k = 0; k < KR; ++k) {
            if (k < K) {
                v[k] = __expf(v[k] - mx);
                se += v[k];
            }
        }
        const float rse = 1.f / se;
        float s = 0.f;                    // sum_j g_j p_j
#pragma unroll
        for (int k = 0; k < KR; ++k) {
            if (k < K) {
                v[k] *= rse;
                s += (coef[K + k] * v[k] + (k == lab ? coef[k] : 0.f)) * v[k];
            }
        }
#pragma unroll
        for (int k = 0; k < KR; ++k) {
            if (k < K) d[k] = v[k] * ((coef[K + k] * v[k] + (k == lab ? coef[k] : 0.f)) - s);
        }
    }
    __syncthreads();
    tile_gather_x(dbuf, lam, pstart, tmp + ((long)b * H + y) * w * K, K, j0, j1, w, npx);
}

// ------------------------------------------------------------------------------------------------ Tversky + binary cross-entropy, fused with the upsample
// CompoundLoss([TverskyLoss(alpha, eps), BinaryCrossEntropyLoss()], [w_t, w_b]) (reference core/models/classifiers/attn/loss.py:7-27, 42-74) on
// z = bilinear(low) for ONE channel, y = mask in [0, 1] (may be soft), p = sigmoid(z), q = p (1 - p), N = B H W:
//   TP = sum p y, FN = sum y (1 - p), FP = sum p (1 - y) over the whole batch;  D = TP + alpha FN + (1 - alpha) FP + eps
//   tversky = 1 - (TP + eps) / D;  bce = 1/N sum [max(z, 0) - z y + log1p(exp(-|z|))];  loss = w_t tversky + w_b bce
//   d loss / d z = w_t q (c1 - c0 y) + w_b / N (p - y),  c0 = 1 / D, c1 = (1 - alpha)(TP + eps) / D^2      (dD/dz = (1 - alpha) q whatever y is)
// The launches of mi_upsample_gdl with K = 1:  tvb_reduce_kernel (per-workgroup partial TP / FN / FP / bce) -> tvb_finalize_kernel (one workgroup: the
// loss and w_t c0, w_t c1, w_b / N in device memory) -> tvb_grad_kernel (d loss / d z gathered along x: tile_stage / tile_gather_x) -> upce_pass2_kernel.
// exp(-|z|) <= 1 everywhere, so saturated logits stay finite; 1 - p is formed from the same exponential, not by subtraction.
constexpr int TVB_NC = 4;          // TP, FN, FP, the bce sum

__device__ __forceinline__ double wave_sum(double v) {
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// p = sigmoid(z), np = 1 - p, e = exp(-|z|)
__device__ __forceinline__ void sigmoid_pair(float z, float& p, float& np, float& e) {
    e = __expf(-fabsf(z));
    const float r = 1.f / (1.f + e), er = e * r;
    p = z >= 0.f ? r : er;
    np = z >= 0.f ? er : r;
}

// The grid of gdl_reduce_kernel: one workgroup per (b, `rows` output rows, GDL_XT output columns), a thread keeps one column and walks the rows.
// partial: [workgroup][4] floats.
__global__ __launch_bounds__(256) void tvb_reduce_kernel(const float* __restrict__ low, const float* __restrict__ mask, float* __restrict__ partial, Axis ay,
                                                         Axis ax, int rows) {
    __shared__ float vrow[GDL_XT + 2];          // source row already interpolated along y
    __shared__ float red[4][TVB_NC];
    const int H = ay.n_out, W = ax.n_out, h = ay.n_in, w = ax.n_in;
    const int tid = threadIdx.x, b = blockIdx.z;
    const int xa = blockIdx.x * GDL_XT, xb = min(W, xa + GDL_XT);
    const int ya = blockIdx.y * rows, yb = min(H, ya + rows);
    int cbase, clast, unused;
    float lx = 0.f;
    ax.src(xa, cbase, unused, lx);
    ax.src(xb - 1, unused, clast, lx);
    const int ncol = min(clast - cbase + 1, GDL_XT + 2);      // upsampling: x0 advances by at most one per pixel
    const int x = xa + tid;
    int x0 = cbase, x1 = cbase;
    if (x < xb) ax.src(x, x0, x1, lx);
    float tp = 0.f, fn = 0.f, fp = 0.f, bce = 0.f;
    for (int y = ya; y < yb; ++y) {
        int y0, y1;
        float ly;
        ay.src(y, y0, y1, ly);
        const float* row0 = low + ((long)b * h + y0) * w + cbase;
        const float* row1 = low + ((long)b * h + y1) * w + cbase;
        for (int e = tid; e < ncol; e += 256) vrow[e] = (1.f - ly) * row0[e] + ly * row1[e];
        __syncthreads();
        if (x < xb) {
            const float t = mask[((long)b * H + y) * W + x];
            const float z = (1.f - lx) * vrow[x0 - cbase] + lx * vrow[x1 - cbase];
            float p, np, e;
            sigmoid_pair(z, p, np, e);
            tp += p * t;
            fn += t * np;
            fp += p * (1.f - t);
            bce += (fmaxf(z, 0.f) - z * t) + log1pf(e);
        }
        __syncthreads();          // the next row overwrites vrow
    }
    const int lane = tid & 63, wv = tid >> 6;
    tp = wave_sum(tp), fn = wave_sum(fn), fp = wave_sum(fp), bce = wave_sum(bce);
    if (lane == 0) {
        red[wv][0] = tp;
        red[wv][1] = fn;
        red[wv][2] = fp;
        red[wv][3] = bce;
    }
    __syncthreads();
    if (tid < TVB_NC) {
        const long wg = ((long)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        partial[wg * TVB_NC + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    }
}

// One workgroup: the partial rows added in fp64 in a fixed order (thread t takes rows t, t + 256, ...; butterfly per wave; the four waves in order), then
// loss_out = loss, tversky, bce, 0; coef = w_t c0, w_t c1, w_b / N; sums (nullable) = TP, FN, FP.
__global__ __launch_bounds__(256) void tvb_finalize_kernel(const float* __restrict__ partial, int n, double npix, float alpha, float eps, float w_t, float w_b,
                                                           float* __restrict__ loss_out, float* __restrict__ coef, float* __restrict__ sums) {
    __shared__ double red[4][TVB_NC];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    double s[TVB_NC] = {0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < n; i += 256) {
        const float4 v = reinterpret_cast<const float4*>(partial)[i];
        s[0] += (double)v.x;
        s[1] += (double)v.y;
        s[2] += (double)v.z;
        s[3] += (double)v.w;
    }
#pragma unroll
    for (int c = 0; c < TVB_NC; ++c) {
        s[c] = wave_sum(s[c]);
        if (lane == 0) red[wv][c] = s[c];
    }
    __syncthreads();
    if (tid == 0) {
        double tot[TVB_NC];
        for (int c = 0; c < TVB_NC; ++c) tot[c] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
        const double a = (double)alpha, e = (double)eps, tpe = tot[0] + e;
        const double D = tot[0] + a * tot[1] + (1.0 - a) * tot[2] + e;          // >= eps > 0
        const double tversky = 1.0 - tpe / D, bce = tot[3] / npix;
        loss_out[0] = (float)((double)w_t * tversky + (double)w_b * bce);
        loss_out[1] = (float)tversky;
        loss_out[2] = (float)bce;
        loss_out[3] = 0.f;
        coef[0] = (float)((double)w_t / D);
        coef[1] = (float)((double)w_t * (1.0 - a) * tpe / (D * D));
        coef[2] = (float)((double)w_b / npix);
        if (sums) {
            sums[0] = (float)tot[0];
            sums[1] = (float)tot[1];
            sums[2] = (float)tot[2];
        }
    }
}

// The tiling of gdl_grad_kernel with one channel: d = d loss / d z from the three coefficients the finalize left in `coef`.
__global__ __launch_bounds__(256) void tvb_grad_kernel(const float* __restrict__ low, const float* __restrict__ mask, const float* __restrict__ coef,
                                                       float* __restrict__ tmp, Axis ay, Axis ax, int npx_max, int jt_cols) {
    extern __shared__ __attribute__((aligned(16))) float sh[];
    float* dbuf = sh;                                           // [npx_max]
    float* lam = sh + npx_max;                                  // [npx_max]  lambda_x
    int* pstart = reinterpret_cast<int*>(lam + npx_max);        // [JT+3] first pixel (relative to xa) whose x0 >= j0 - 1 + q
    float* vrow = reinterpret_cast<float*>(pstart + JT + 4);    // [JT+2] low-res row already interpolated along y
    const int H = ay.n_out, W = ax.n_out, w = ax.n_in;
    const int jt = blockIdx.x, y = blockIdx.y, b = blockIdx.z;
    const int j0 = jt * jt_cols, j1 = min(w, j0 + jt_cols);
    const int xa = ax.first_with_i0_ge(j0 - 1), xb = ax.first_with_i0_ge(j1);   // pixels with x0 in [j0-1, j1-1]
    const int npx = min(xb - xa, npx_max);
    int cbase;
    tile_stage(low, 1, ay, ax, b, y, j0, j1, xa, pstart, vrow, cbase);
    __syncthreads();
    const float c0 = coef[0], c1 = coef[1], cb = coef[2];
    for (int px = threadIdx.x; px < npx; px += 256) {
        const int x = xa + px;
        int x0, x1;
        float lx;
        ax.src(x, x0, x1, lx);
        lam[px] = lx;
        const float t = mask[((long)b * H + y) * W + x];
        const float z = (1.f - lx) * vrow[x0 - cbase] + lx * vrow[x1 - cbase];
        float p, np, e;
        sigmoid_pair(z, p, np, e);
        dbuf[px] = (p * np) * (c1 - c0 * t) + cb * (p - t);
    }
    __syncthreads();
    tile_gather_x(dbuf, lam, pstart, tmp + ((long)b * H + y) * w, 1, j0, j1, w, npx);
}

// ------------------------------------------------------------------------------------------------ inference tails
// The per-source arithmetic of both inference tails: the bilinear (align_corners) sample of the NHWC map `low` (one image) at output pixel
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
    float se = 0.f;
#pragma unroll
    for (int k = 0; k < KR; ++k) {
        if (k < K) {
            v[k] = __expf(v[k] - mx);
            se += v[k];
        }
    }
    return 1.f / se;
}

// probs NCHW + optional argmax
__global__ void upsample_softmax_kernel(const float* __restrict__ low, float* __restrict__ probs, uint8_t* __restrict__ pred, int B, int K,
                                        Axis ay, Axis ax) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int H = ay.n_out, W = ax.n_out, h = ay.n_in, w = ax.n_in;
    if (idx >= (long)B * H * W) return;
    const int x = (int)(idx % W), y = (int)((idx / W) % H), b = (int)(idx / ((long)W * H));
    float v[KMAX];
    int arg;
    const float rse = interp_softmax_terms<KMAX>(low + (long)b * h * w * K, K, ay, ax, y, x, v, arg);
    float* o = probs + ((long)b * K * H + y) * W + x;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        if (k < K) o[(long)k * H * W] = v[k] * rse;
    }
    if (pred) pred[idx] = (uint8_t)arg;
}

// Multi-scale, flip-averaged tail (reference core/utils/utility.py:193-209): probs = ((p_0 + ... + p_{n-1}) / div_a) / div_b with
// p_i = softmax(bilinear(low_i -> H x W)), read at column W-1-x for a mirrored source.  The reference adds materialised fp32 tensors, so every
// p_i[k] is a rounded product before it is added (no fma), the sum runs in source order and the divisions are true divisions.
// One thread owns P consecutive pixels of a row (2 when W is even, else 1) and keeps their K sums in registers; each class plane is written once.
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

// The per-pixel arithmetic of the multi-scale tails, shared by the probability kernel and the predict-and-score kernel so that the two cannot
// drift apart: acc[p][k] = ((p_0 + ... + p_{n-1}) / div_a) / div_b for the P pixels (y, xb .. xb+P-1), summed in source order from rounded
// products, with true divisions (the second one skipped when div_b == 1).
template <int KR, int P>
__device__ __forceinline__ void multi_probs(const ProbSrcs& srcs, int n, int K, int W, int y, int xb, float div_a, float div_b, float (&acc)[P][KR]) {
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
        for (int k = 0; k < KR; ++k) acc[p][k] = 0.f;      // 0 + p_0 == p_0 exactly (p_0 >= +0)
    for (int i = 0; i < n; ++i) {
        const ProbSrc& s = srcs.s[i];
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

// Waves per SIMD the register budget is held to.  A pixel has 4 x K corner loads in flight besides the P x K sums: one pixel per lane runs at
// 4 waves, two pixels per lane (8-byte stores, 512 contiguous bytes per wave and class plane) at 2.  Four pixels per lane spill.  No variant here does.
template <int KT, int P>
__global__ __launch_bounds__(256, P == 1 ? 4 : 2) void upsample_softmax_multi_kernel(ProbSrcs srcs, int n, float* __restrict__ probs, int Krt, int H, int W,
                                                                     float div_a, float div_b) {
    const int K = KT > 0 ? KT : Krt;
    constexpr int KR = KT > 0 ? KT : KMAX;
    static_assert(P == 1 || P == 2, "one or two pixels per lane");
    const int WP = W / P;                                  // P == 2 only when W is even
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)H * WP) return;
    const int xb = (int)(idx % WP) * P, y = (int)(idx / WP);
    float acc[P][KR];
    multi_probs<KR, P>(srcs, n, K, W, y, xb, div_a, div_b, acc);
    float* o = probs + (long)y * W + xb;
#pragma unroll
    for (int k = 0; k < KR; ++k) {
        if (k < K) {
            float* ok = o + (long)k * H * W;
            if constexpr (P == 2)
                *reinterpret_cast<float2*>(ok) = make_float2(acc[0][k], acc[1][k]);        // W even and probs 8-byte aligned (the launcher checks)
            else
                ok[0] = acc[0][k];
        }
    }
}

// Evaluation tail without the probability map: the same K values per pixel as upsample_softmax_multi_kernel (multi_probs), reduced in registers to
// pred = the LOWEST class index among their maxima (torch.max(dim) / numpy.argmax), pseudo = max >= threshold ? pred : 255, and - with labels -
// the integers host/metrics.py derives from pred.  One LDS add per pixel: cell gt * K + pd where the label gt lies in [0, K) (confusion_matrix;
// 255 and ignore_index lie outside [0, K)), cell K * K + pd where it does not and is not ignore_index.  From these, per class k:
//   area_intersection = cmt[k][k], area_target = row sum k, area_output = column sum k + the extra cell k.
// A workgroup sees at most 512 pixels, so its 32-bit LDS counters cannot overflow; it flushes one 64-bit global add per non-zero cell.  Integer sums
// do not depend on arrival order: the counts are bit-reproducible.  counts: [K*K] cmt, [K] intersection, [K] output, [K] target; added to.
template <int KT, int P>
__global__ __launch_bounds__(256, P == 1 ? 4 : 2) void upsample_predict_score_kernel(ProbSrcs srcs, int n, int Krt, int H, int W, float div_a, float div_b,
                                                                     const long long* __restrict__ labels, int ignore_index, float threshold,
                                                                     uint8_t* __restrict__ pred, uint8_t* __restrict__ pseudo,
                                                                     unsigned long long* __restrict__ counts) {
    const int K = KT > 0 ? KT : Krt;
    constexpr int KR = KT > 0 ? KT : KMAX;
    static_assert(P == 1 || P == 2, "one or two pixels per lane");
    __shared__ unsigned tab[KR * KR + KR];
    const int tid = threadIdx.x;
    if (counts) {                                          // uniform over the grid
        for (int c = tid; c < K * K + K; c += 256) tab[c] = 0u;
        __syncthreads();
    }
    const int WP = W / P;                                  // P == 2 only when W is even
    const long idx = (long)blockIdx.x * 256 + tid;
    if (idx < (long)H * WP) {
        const int xb = (int)(idx % WP) * P, y = (int)(idx / WP);
        float acc[P][KR];
        multi_probs<KR, P>(srcs, n, K, W, y, xb, div_a, div_b, acc);
        uint8_t pd[P], ps[P];
#pragma unroll
        for (int p = 0; p < P; ++p) {
            float best = acc[p][0];
            int arg = 0;
#pragma unroll
            for (int k = 1; k < KR; ++k) {
                if (k < K && acc[p][k] > best) {           // strict: the first of equal maxima stays
                    best = acc[p][k];
                    arg = k;
                }
            }
            pd[p] = (uint8_t)arg;
            ps[p] = best >= threshold ? (uint8_t)arg : (uint8_t)255;
        }
        const long o = (long)y * W + xb;
        if constexpr (P == 2) {                            // W even: o even; pred / pseudo 2-byte, labels 16-byte aligned (the launcher checks)
            *reinterpret_cast<uchar2*>(pred + o) = make_uchar2(pd[0], pd[1]);
            if (pseudo) *reinterpret_cast<uchar2*>(pseudo + o) = make_uchar2(ps[0], ps[1]);
        } else {
            pred[o] = pd[0];
            if (pseudo) pseudo[o] = ps[0];
        }
        if (counts) {
            long long gt[P];
            if constexpr (P == 2) {
                const longlong2 g = *reinterpret_cast<const longlong2*>(labels + o);
                gt[0] = g.x;
                gt[1] = g.y;
            } else {
                gt[0] = labels[o];
            }
#pragma unroll
            for (int p = 0; p < P; ++p) {
                if ((unsigned long long)gt[p] < (unsigned long long)K)
                    atomicAdd(&tab[(int)gt[p] * K + pd[p]], 1u);
                else if (gt[p] != (long long)ignore_index)
                    atomicAdd(&tab[K * K + pd[p]], 1u);
            }
        }
    }
    if (counts) {
        __syncthreads();
        for (int c = tid; c < K * K; c += 256) {
            const unsigned v = tab[c];
            if (v) atomicAdd(&counts[c], (unsigned long long)v);
        }
        if (tid < K) {
            unsigned row = 0u, col = 0u;
            for (int j = 0; j < K; ++j) {
                row += tab[tid * K + j];
                col += tab[j * K + tid];
            }
            const unsigned diag = tab[tid * K + tid], out = col + tab[K * K + tid];
            if (diag) atomicAdd(&counts[K * K + tid], (unsigned long long)diag);
            if (out) atomicAdd(&counts[K * K + K + tid], (unsigned long long)out);
            if (row) atomicAdd(&counts[K * K + 2 * K + tid], (unsigned long long)row);
        }
    }
}

// F.interpolate(x, (Ho, Wo), mode='bilinear', align_corners=True) on NCHW fp32 images; with_mirror: image b's horizontal mirror
// (torch.flip(resized, [3])) is written as image B + b from the same registers, so the two halves are bit-equal mirrors.
__global__ void image_resize_ac_kernel(const float* __restrict__ x, float* __restrict__ out, int B, int C, Axis ay, Axis ax, int with_mirror) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int Ho = ay.n_out, Wo = ax.n_out, H = ay.n_in, W = ax.n_in;
    if (idx >= (long)B * C * Ho * Wo) return;
    const int xo = (int)(idx % Wo), yo = (int)((idx / Wo) % Ho);
    const long bc = idx / ((long)Wo * Ho);
    int y0, y1, x0, x1;
    float ly, lx;
    ay.src(yo, y0, y1, ly);
    ax.src(xo, x0, x1, lx);
    const float* p = x + bc * H * W;
    const float v00 = p[(long)y0 * W + x0];
    // on a grid point (every pixel when the size does not change) the value is the input's, bit for bit (-0 and non-finite neighbours included)
    const float val = (lx == 0.f && ly == 0.f) ? v00 : lerp2(v00, p[(long)y0 * W + x1], p[(long)y1 * W + x0], p[(long)y1 * W + x1], lx, ly);
    out[idx] = val;
    if (with_mirror) out[((bc + (long)B * C) * Ho + yo) * Wo + (Wo - 1 - xo)] = val;
}

inline unsigned nblk(long n, int bs) { return (unsigned)((n + bs - 1) / bs); }

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

}  // namespace

extern "C" int mi_upsample_ac_fwd(const float* low, float* up, int B, int h, int w, int K, int H, int W, void* stream) {
    MI_REQUIRE(low && up && B > 0 && h > 0 && w > 0 && K > 0 && H > 0 && W > 0, "mi_upsample_ac_fwd: bad argument");
    hipLaunchKernelGGL(upsample_fwd_kernel, dim3(nblk((long)B * H * W, 256)), dim3(256), 0, (hipStream_t)stream, low, up, B, K, make_axis(h, H),
                       make_axis(w, W));
    MI_CHECK_LAUNCH("mi_upsample_ac_fwd");
    return MI_OK;
}

extern "C" int mi_upsample_ac_bwd(const float* dup, float* dlow, int B, int h, int w, int K, int H, int W, void* stream) {
    MI_REQUIRE(dup && dlow && B > 0 && h > 0 && w > 0 && K > 0 && H > 0 && W > 0, "mi_upsample_ac_bwd: bad argument");
    hipLaunchKernelGGL(upsample_bwd_kernel, dim3(nblk((long)B * K * h * w, 256)), dim3(256), 0, (hipStream_t)stream, dup, dlow, B, K,
                       make_axis(h, H), make_axis(w, W));
    MI_CHECK_LAUNCH("mi_upsample_ac_bwd");
    return MI_OK;
}

extern "C" size_t mi_ce_workspace(int B, int H, int W) { return (size_t)nblk((long)B * H * W, 256) * 2 * sizeof(float); }

extern "C" int mi_softmax_ce_fwd(const float* logits, const int64_t* labels, float* loss_out, int B, int K, int H, int W, int ignore_index,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    MI_REQUIRE(logits && labels && loss_out && workspace && B > 0 && K > 0 && H > 0 && W > 0, "mi_softmax_ce_fwd: bad argument");
    if (workspace_bytes < mi_ce_workspace(B, H, W)) return mi_set_error(MI_ENOMEM, "mi_softmax_ce_fwd: workspace too small");
    const unsigned nb = nblk((long)B * H * W, 256);
    unsigned* bad = reinterpret_cast<unsigned*>(loss_out + 3);
    if (hipMemsetAsync(bad, 0, sizeof(unsigned), (hipStream_t)stream) != hipSuccess) return mi_set_error(MI_EHIP, "mi_softmax_ce_fwd: memset");
    hipLaunchKernelGGL(ce_fwd_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, logits, labels, (float*)workspace, B, K, (long)H * W, ignore_index, bad);
    MI_CHECK_LAUNCH("mi_softmax_ce_fwd");
    hipLaunchKernelGGL(ce_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, (int)nb, loss_out);
    MI_CHECK_LAUNCH("mi_softmax_ce_fwd finalize");
    return MI_OK;
}

extern "C" int mi_softmax_ce_bwd(const float* logits, const int64_t* labels, const float* loss_out, float* dlogits, int B, int K, int H, int W,
                                 int ignore_index, float grad_scale, void* stream) {
    MI_REQUIRE(logits && labels && loss_out && dlogits && B > 0 && K > 0 && H > 0 && W > 0, "mi_softmax_ce_bwd: bad argument");
    hipLaunchKernelGGL(ce_bwd_kernel, dim3(nblk((long)B * H * W, 256)), dim3(256), 0, (hipStream_t)stream, logits, labels, loss_out, dlogits, B, K,
                       (long)H * W, ignore_index, grad_scale);
    MI_CHECK_LAUNCH("mi_softmax_ce_bwd");
    return MI_OK;
}

extern "C" size_t mi_upsample_ce_workspace(int B, int h, int w, int K, int H, int W) {
    const int jt_cols = pick_jt(w, W);
    const size_t tiles = (size_t)((w + jt_cols - 1) / jt_cols);
    const size_t partial = (size_t)B * H * tiles * 2 * sizeof(float);
    const size_t tmp = (size_t)B * H * w * K * sizeof(float);
    return ((partial + 255) & ~(size_t)255) + tmp;
}

extern "C" int mi_upsample_ce_ex(const float* low, const int64_t* labels, float* loss_out, float* dlow, int B, int h, int w, int K, int H, int W,
                                 int ignore_index, float grad_scale, int align_corners, void* workspace, size_t workspace_bytes, void* stream);

extern "C" int mi_upsample_ce(const float* low, const int64_t* labels, float* loss_out, float* dlow, int B, int h, int w, int K, int H, int W,
                              int ignore_index, float grad_scale, void* workspace, size_t workspace_bytes, void* stream) {
    return mi_upsample_ce_ex(low, labels, loss_out, dlow, B, h, w, K, H, W, ignore_index, grad_scale, 1, workspace, workspace_bytes, stream);
}

extern "C" int mi_upsample_ce_ex(const float* low, const int64_t* labels, float* loss_out, float* dlow, int B, int h, int w, int K, int H, int W,
                                 int ignore_index, float grad_scale, int align_corners, void* workspace, size_t workspace_bytes, void* stream) {
    MI_REQUIRE(low && labels && loss_out && workspace, "mi_upsample_ce: null operand");
    MI_REQUIRE(B > 0 && h > 0 && w > 0 && H > 0 && W > 0 && K > 0 && K <= KMAX, "mi_upsample_ce: bad dimension (K <= 32)");
    MI_REQUIRE(H >= h && W >= w, "mi_upsample_ce: only upsampling (H >= h, W >= w) is supported");
    MI_REQUIRE(H <= 65535 && B <= 65535, "mi_upsample_ce: grid dimension overflow");
    if (workspace_bytes < mi_upsample_ce_workspace(B, h, w, K, H, W)) return mi_set_error(MI_ENOMEM, "mi_upsample_ce: workspace too small");
    const Axis ay = make_axis(h, H, align_corners), ax = make_axis(w, W, align_corners);
    const int jt_cols = pick_jt(w, W);
    const int tiles = (w + jt_cols - 1) / jt_cols;
    float* partial = (float*)workspace;
    const size_t poff = (((size_t)B * H * tiles * 2 * sizeof(float)) + 255) & ~(size_t)255;
    float* tmp = dlow ? (float*)((char*)workspace + poff) : nullptr;
    const int npx_max = pass1_npx_max(ax, jt_cols);
    const size_t lds = (size_t)npx_max * K * 4 + (size_t)npx_max * 8 + 512 * 4 + (JT + 4) * 4 + (size_t)(JT + 2) * K * 4;
    MI_REQUIRE(lds <= 160 * 1024, "mi_upsample_ce: upsample factor too large for one LDS tile (%zu B)", lds);
    static std::atomic<uint64_t> lds_set[2];           // the launch size varies with the upsample factor: allow the maximum once per device
    mi_allow_dynamic_lds((const void*)upce_pass1_kernel<19>, MI_LDS_MAX, lds_set[0]);
    mi_allow_dynamic_lds((const void*)upce_pass1_kernel<0>, MI_LDS_MAX, lds_set[1]);
    unsigned* bad = reinterpret_cast<unsigned*>(loss_out + 3);
    if (hipMemsetAsync(bad, 0, sizeof(unsigned), (hipStream_t)stream) != hipSuccess) return mi_set_error(MI_EHIP, "mi_upsample_ce: memset");
    if (K == 19)
        hipLaunchKernelGGL(upce_pass1_kernel<19>, dim3(tiles, H, B), dim3(256), lds, (hipStream_t)stream, low, labels, partial, tmp, B, K, ay,
                           ax, ignore_index, npx_max, bad, jt_cols, WceArgs{nullptr, 1.f, 0.f});
    else
        hipLaunchKernelGGL(upce_pass1_kernel<0>, dim3(tiles, H, B), dim3(256), lds, (hipStream_t)stream, low, labels, partial, tmp, B, K, ay,
                           ax, ignore_index, npx_max, bad, jt_cols, WceArgs{nullptr, 1.f, 0.f});
    MI_CHECK_LAUNCH("mi_upsample_ce pass1");
    hipLaunchKernelGGL(ce_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)partial, B * H * tiles, loss_out);
    MI_CHECK_LAUNCH("mi_upsample_ce finalize");
    if (dlow) {
        hipLaunchKernelGGL(upce_pass2_kernel, dim3(nblk((long)B * h * w * K, 256)), dim3(256), 0, (hipStream_t)stream, (const float*)tmp, loss_out,
                           dlow, B, K, ay, w, grad_scale);
        MI_CHECK_LAUNCH("mi_upsample_ce pass2");
    }
    return MI_OK;
}

// CrossEntropyLoss(weight=, ignore_index=, label_smoothing=) on the upsampled logits: the launches of mi_upsample_ce_ex with the weighted
// instantiation of pass 1 (the weights travel as a device pointer, so a captured graph sees later values) and the pass 2 that keeps exact zeros.
// Without weights and smoothing pass 1 is the PLAIN instantiation, the very code mi_upsample_ce_ex launches: the compiler contracts the two
// instantiations differently (the plain <19> interpolates with two rounded products, the weighted one with an fma), so only the same code object
// makes "the defaults give mi_upsample_ce_ex's bits" hold whatever a later compiler does.
extern "C" int mi_upsample_ce_w(const float* low, const int64_t* labels, const float* class_weights, float* loss_out, float* dlow, int B, int h, int w,
                                int K, int H, int W, int ignore_index, float label_smoothing, float grad_scale, int align_corners, void* workspace,
                                size_t workspace_bytes, void* stream) {
    MI_REQUIRE(low && labels && loss_out && workspace, "mi_upsample_ce_w: null operand");
    MI_REQUIRE(B > 0 && h > 0 && w > 0 && H > 0 && W > 0 && K > 0 && K <= KMAX, "mi_upsample_ce_w: bad dimension (K <= 32)");
    MI_REQUIRE(H >= h && W >= w, "mi_upsample_ce_w: only upsampling (H >= h, W >= w) is supported");
    MI_REQUIRE(H <= 65535 && B <= 65535, "mi_upsample_ce_w: grid dimension overflow");
    MI_REQUIRE(std::isfinite(label_smoothing), "mi_upsample_ce_w: label_smoothing is not finite");
    MI_REQUIRE(label_smoothing >= 0.f && label_smoothing <= 1.f, "mi_upsample_ce_w: label_smoothing outside [0, 1]");
    MI_REQUIRE(std::isfinite(grad_scale), "mi_upsample_ce_w: grad_scale is not finite");
    if (workspace_bytes < mi_upsample_ce_workspace(B, h, w, K, H, W)) return mi_set_error(MI_ENOMEM, "mi_upsample_ce_w: workspace too small");
    const Axis ay = make_axis(h, H, align_corners), ax = make_axis(w, W, align_corners);
    const int jt_cols = pick_jt(w, W);
    const int tiles = (w + jt_cols - 1) / jt_cols;
    float* partial = (float*)workspace;
    const size_t poff = (((size_t)B * H * tiles * 2 * sizeof(float)) + 255) & ~(size_t)255;
    float* tmp = dlow ? (float*)((char*)workspace + poff) : nullptr;
    const int npx_max = pass1_npx_max(ax, jt_cols);
    const bool plain = !class_weights && label_smoothing == 0.f;
    const size_t lds = (size_t)npx_max * K * 4 + (size_t)npx_max * 8 + 512 * 4 + (JT + 4) * 4 + (size_t)(JT + 2) * K * 4 + (plain ? 0 : (size_t)(K + 1) * 4);
    MI_REQUIRE(lds <= 160 * 1024, "mi_upsample_ce_w: upsample factor too large for one LDS tile (%zu B)", lds);
    static std::atomic<uint64_t> lds_set[4];
    mi_allow_dynamic_lds((const void*)upce_pass1_kernel<19, UPCE_WEIGHTED>, MI_LDS_MAX, lds_set[0]);
    mi_allow_dynamic_lds((const void*)upce_pass1_kernel<0, UPCE_WEIGHTED>, MI_LDS_MAX, lds_set[1]);
    mi_allow_dynamic_lds((const void*)upce_pass1_kernel<19>, MI_LDS_MAX, lds_set[2]);
    mi_allow_dynamic_lds((const void*)upce_pass1_kernel<0>, MI_LDS_MAX, lds_set[3]);
    const WceArgs wce{class_weights, 1.f - label_smoothing, label_smoothing / (float)K};
    unsigned* bad = reinterpret_cast<unsigned*>(loss_out + 3);
    if (hipMemsetAsync(bad, 0, sizeof(unsigned), (hipStream_t)stream) != hipSuccess) return mi_set_error(MI_EHIP, "mi_upsample_ce_w: memset");
    if (plain && K == 19)
        hipLaunchKernelGGL(upce_pass1_kernel<19>, dim3(tiles, H, B), dim3(256), lds, (hipStream_t)stream, low, labels, partial, tmp, B, K, ay, ax, ignore_index,
                           npx_max, bad, jt_cols, wce);
    else if (plain)
        hipLaunchKernelGGL(upce_pass1_kernel<0>, dim3(tiles, H, B), dim3(256), lds, (hipStream_t)stream, low, labels, partial, tmp, B, K, ay, ax, ignore_index,
                           npx_max, bad, jt_cols, wce);
    else if (K == 19)
        hipLaunchKernelGGL((upce_pass1_kernel<19, UPCE_WEIGHTED>), dim3(tiles, H, B), dim3(256), lds, (hipStream_t)stream, low, labels, partial, tmp, B, K,
                           ay, ax, ignore_index, npx_max, bad, jt_cols, wce);
    else
        hipLaunchKernelGGL((upce_pass1_kernel<0, UPCE_WEIGHTED>), dim3(tiles, H, B), dim3(256), lds, (hipStream_t)stream, low, labels, partial, tmp, B, K,
                           ay, ax, ignore_index, npx_max, bad, jt_cols, wce);
    MI_CHECK_LAUNCH("mi_upsample_ce_w pass1");
    hipLaunchKernelGGL(ce_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)partial, B * H * tiles, loss_out);
    MI_CHECK_LAUNCH("mi_upsample_ce_w finalize");
    if (dlow) {
        hipLaunchKernelGGL(wce_pass2_kernel, dim3(nblk((long)B * h * w * K, 256)), dim3(256), 0, (hipStream_t)stream, (const float*)tmp, loss_out, dlow, B, K,
                           ay, w, grad_scale);
        MI_CHECK_LAUNCH("mi_upsample_ce_w pass2");
    }
    return MI_OK;
}

namespace {
// The reduction pass's grid: GDL_XT-column tiles, and as many rows per workgroup as keep the launch near 1024 workgroups (4 per CU, what the kernel's
// registers let a CU hold: one round; and the partial rows the one-workgroup finalize has to add stay a few hundred KB at 6 x 720 x 1280).
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
inline size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }
}  // namespace

extern "C" size_t mi_upsample_gdl_workspace(int B, int h, int w, int K, int H, int W) {
    if (B <= 0 || h <= 0 || w <= 0 || K <= 0 || H <= 0 || W <= 0) return 0;
    const GdlPlan p = gdl_plan(B, H, W);
    return up256(p.nwg * (3 * (size_t)K + 1) * sizeof(unsigned)) + up256(2 * (size_t)K * sizeof(float)) + (size_t)B * H * w * K * sizeof(float);
}

extern "C" int mi_upsample_gdl(const float* low, const int64_t* labels, float* loss_out, float* dlow, float* sums, int B, int h, int w, int K, int H,
                               int W, int ignore_index, int weight_type, float eps, float grad_scale, int align_corners, void* workspace,
                               size_t workspace_bytes, void* stream) {
    MI_REQUIRE(low && labels && loss_out && workspace, "mi_upsample_gdl: null operand");
    MI_REQUIRE(B > 0 && h > 0 && w > 0 && H > 0 && W > 0 && K > 0 && K <= KMAX, "mi_upsample_gdl: bad dimension (K <= 32)");
    MI_REQUIRE(H >= h && W >= w, "mi_upsample_gdl: only upsampling (H >= h, W >= w) is supported");
    MI_REQUIRE(H <= 65535 && B <= 65535, "mi_upsample_gdl: grid dimension overflow");
    MI_REQUIRE(weight_type >= MI_GDL_SQUARE && weight_type <= MI_GDL_SQRT, "mi_upsample_gdl: weight_type is MI_GDL_SQUARE, MI_GDL_IDENTITY or MI_GDL_SQRT");
    MI_REQUIRE(eps > 0.f, "mi_upsample_gdl: eps must be positive");
    if (workspace_bytes < mi_upsample_gdl_workspace(B, h, w, K, H, W)) return mi_set_error(MI_ENOMEM, "mi_upsample_gdl: workspace too small");
    const Axis ay = make_axis(h, H, align_corners), ax = make_axis(w, W, align_corners);
    const GdlPlan pl = gdl_plan(B, H, W);
    unsigned* partial = (unsigned*)workspace;
    float* coef = (float*)((char*)workspace + up256(pl.nwg * (3 * (size_t)K + 1) * sizeof(unsigned)));
    float* tmp = (float*)((char*)coef + up256(2 * (size_t)K * sizeof(float)));
    const int ncol_max = w < GDL_XT + 2 ? w : GDL_XT + 2;
    const size_t lds1 = ((size_t)ncol_max * K + 4 * (3 * (size_t)K + 1)) * 4;          // <= 34 KB
    const int jt_cols = pick_jt(w, W);
    const int npx_max = pass1_npx_max(ax, jt_cols);
    const size_t lds3 = (size_t)npx_max * K * 4 + (size_t)npx_max * 4 + (JT + 4) * 4 + (size_t)(JT + 2) * K * 4;
    MI_REQUIRE(!dlow || lds3 <= 160 * 1024, "mi_upsample_gdl: upsample factor too large for one LDS tile (%zu B)", lds3);
    const dim3 g1(pl.tiles_x, pl.row_groups, B);
    if (K == 19)
        hipLaunchKernelGGL(gdl_reduce_kernel<19>, g1, dim3(256), lds1, (hipStream_t)stream, low, labels, partial, K, ay, ax, ignore_index, pl.rows, ncol_max);
    else
        hipLaunchKernelGGL(gdl_reduce_kernel<0>, g1, dim3(256), lds1, (hipStream_t)stream, low, labels, partial, K, ay, ax, ignore_index, pl.rows, ncol_max);
    MI_CHECK_LAUNCH("mi_upsample_gdl reduce");
    hipLaunchKernelGGL(gdl_finalize_kernel, dim3(1), dim3(64 * GDL_FIN_WAVES), 0, (hipStream_t)stream, (const unsigned*)partial, (int)pl.nwg, K, weight_type, eps, loss_out,
                       coef, sums);
    MI_CHECK_LAUNCH("mi_upsample_gdl finalize");
    if (dlow) {
        static std::atomic<uint64_t> lds_set[2];
        mi_allow_dynamic_lds((const void*)gdl_grad_kernel<19>, MI_LDS_MAX, lds_set[0]);
        mi_allow_dynamic_lds((const void*)gdl_grad_kernel<0>, MI_LDS_MAX, lds_set[1]);
        const int tiles = (w + jt_cols - 1) / jt_cols;
        if (K == 19)
            hipLaunchKernelGGL(gdl_grad_kernel<19>, dim3(tiles, H, B), dim3(256), lds3, (hipStream_t)stream, low, labels, (const float*)coef, tmp, K, ay, ax,
                               ignore_index, npx_max, jt_cols);
        else
            hipLaunchKernelGGL(gdl_grad_kernel<0>, dim3(tiles, H, B), dim3(256), lds3, (hipStream_t)stream, low, labels, (const float*)coef, tmp, K, ay, ax,
                               ignore_index, npx_max, jt_cols);
        MI_CHECK_LAUNCH("mi_upsample_gdl gradient");
        hipLaunchKernelGGL(upce_pass2_kernel, dim3(nblk((long)B * h * w * K, 256)), dim3(256), 0, (hipStream_t)stream, (const float*)tmp,
                           (const float*)nullptr, dlow, B, K, ay, w, grad_scale);
        MI_CHECK_LAUNCH("mi_upsample_gdl gradient rows");
    }
    return MI_OK;
}

extern "C" size_t mi_upsample_tversky_bce_workspace(int B, int h, int w, int H, int W) {
    if (B <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return 0;
    const GdlPlan p = gdl_plan(B, H, W);
    return up256(p.nwg * TVB_NC * sizeof(float)) + up256(3 * sizeof(float)) + (size_t)B * H * w * sizeof(float);
}

extern "C" int mi_upsample_tversky_bce(const float* low, const float* mask, float* loss_out, float* dlow, float* sums, int B, int h, int w, int H, int W,
                                       float alpha, float eps, float w_tversky, float w_bce, float grad_scale, int align_corners, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    MI_REQUIRE(low && mask && loss_out && workspace, "mi_upsample_tversky_bce: null operand");
    MI_REQUIRE(B > 0 && h > 0 && w > 0 && H > 0 && W > 0, "mi_upsample_tversky_bce: bad dimension");
    MI_REQUIRE(H >= h && W >= w, "mi_upsample_tversky_bce: only upsampling (H >= h, W >= w) is supported");
    MI_REQUIRE(H <= 65535 && B <= 65535, "mi_upsample_tversky_bce: grid dimension overflow");
    MI_REQUIRE(alpha >= 0.f && alpha <= 1.f, "mi_upsample_tversky_bce: alpha outside [0, 1]");          // (a NaN fails both comparisons)
    MI_REQUIRE(eps > 0.f, "mi_upsample_tversky_bce: eps must be positive");
    if (workspace_bytes < mi_upsample_tversky_bce_workspace(B, h, w, H, W)) return mi_set_error(MI_ENOMEM, "mi_upsample_tversky_bce: workspace too small");
    const Axis ay = make_axis(h, H, align_corners), ax = make_axis(w, W, align_corners);
    const GdlPlan pl = gdl_plan(B, H, W);
    float* partial = (float*)workspace;
    float* coef = (float*)((char*)workspace + up256(pl.nwg * TVB_NC * sizeof(float)));
    float* tmp = (float*)((char*)coef + up256(3 * sizeof(float)));
    const int jt_cols = pick_jt(w, W);
    const int npx_max = pass1_npx_max(ax, jt_cols);
    const size_t lds3 = (size_t)npx_max * 8 + (JT + 4) * 4 + (size_t)(JT + 2) * 4;
    MI_REQUIRE(!dlow || lds3 <= 64 * 1024, "mi_upsample_tversky_bce: upsample factor too large for one LDS tile (%zu B)", lds3);
    hipLaunchKernelGGL(tvb_reduce_kernel, dim3(pl.tiles_x, pl.row_groups, B), dim3(256), 0, (hipStream_t)stream, low, mask, partial, ay, ax, pl.rows);
    MI_CHECK_LAUNCH("mi_upsample_tversky_bce reduce");
    hipLaunchKernelGGL(tvb_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)partial, (int)pl.nwg, (double)B * H * W, alpha, eps,
                       w_tversky, w_bce, loss_out, coef, sums);
    MI_CHECK_LAUNCH("mi_upsample_tversky_bce finalize");
    if (dlow) {
        const int tiles = (w + jt_cols - 1) / jt_cols;
        hipLaunchKernelGGL(tvb_grad_kernel, dim3(tiles, H, B), dim3(256), lds3, (hipStream_t)stream, low, mask, (const float*)coef, tmp, ay, ax, npx_max,
                           jt_cols);
        MI_CHECK_LAUNCH("mi_upsample_tversky_bce gradient");
        hipLaunchKernelGGL(upce_pass2_kernel, dim3(nblk((long)B * h * w, 256)), dim3(256), 0, (hipStream_t)stream, (const float*)tmp, (const float*)nullptr,
                           dlow, B, 1, ay, w, grad_scale);
        MI_CHECK_LAUNCH("mi_upsample_tversky_bce gradient rows");
    }
    return MI_OK;
}

namespace {
// ------------------------------------------------------------------------------------------------ online hard example mining, fused with the upsample
// Cross-entropy averaged over the hard pixels only (the OhemCrossEntropy2d of GALDNet / CCNet / OCNet / HRNet-Seg), on z = bilinear(low):
//   q_i = softmax(z_i)[y_i] on valid pixels, n of them;  k = min(min_kept, n);  t = max(thresh, k-th smallest q);  kept_i = valid_i and q_i <= t
//   loss = sum_kept (-log q_i) / n_kept;  d loss / d z_c = kept_i (p_i[c] - [c == y_i]) / n_kept      (nothing differentiates through t)
// Launches (nothing is read back, so the call can be captured):
//   memset of the histograms and counters
//   ohem_prob_kernel      q (2.0 = not valid) and -log q of every full-resolution pixel into the workspace, the counts of valid and out-of-range pixels,
//                         and the histogram of bits 31..21 of q (positive floats order as their unsigned bits).  The grid of gdl_reduce_kernel.
//   ohem_scan_kernel 0    one workgroup: k, prefix scan of the 2048 bins, the bucket that holds the k-th smallest, the rank left inside it
//   ohem_hist_kernel 1    histogram of bits 20..10 of the q whose bits 31..21 equal the chosen bucket;  ohem_scan_kernel 1
//   ohem_hist_kernel 2    histogram of bits 9..0 of the q whose bits 31..10 equal the prefix;            ohem_scan_kernel 2: all 32 bits of the k-th smallest, t
//   ohem_loss_kernel      per-workgroup sum of -log q and count over q <= t;  ohem_finalize_kernel: loss_out
//   ohem_grad_kernel      gdl_grad_kernel's tiling with d = (q <= t) (p - onehot), the decision read from the STORED q: the pixels that receive gradient are
//                         the n_kept that were counted;  wce_pass2_kernel divides by loss_out[1] = n_kept and keeps exact zeros.
// Histograms live in LDS and are merged with integer atomics (order-independent); every float sum has a fixed order: two calls give the same bits.
constexpr int OHEM_BINS = 2048;
constexpr int OHEM_WGS = 1024;          // workgroups of the streaming passes over q (grid-stride)
enum { OHEM_NVALID = 0, OHEM_BAD = 1, OHEM_PREFIX = 2, OHEM_RANK = 3, OHEM_T = 4, OHEM_STATE = 8 };          // the words behind the three histograms
constexpr float OHEM_SENTINEL = 2.f;

template <int KT>
__global__ __launch_bounds__(256) void ohem_prob_kernel(const float* __restrict__ low, const int64_t* __restrict__ labels, float* __restrict__ qout,
                                                        float* __restrict__ nllout, unsigned* __restrict__ hist, unsigned* __restrict__ state, int Krt, Axis ay,
                                                        Axis ax, int ignore_index, int rows, int ncol_max) {
    const int K = KT > 0 ? KT : Krt;
    constexpr int KR = KT > 0 ? KT : KMAX;
    extern __shared__ __attribute__((aligned(16))) float sh[];
    float* vrow = sh;                                                          // [ncol_max][K] source row already interpolated along y
    unsigned* lh = reinterpret_cast<unsigned*>(sh + (long)ncol_max * K);       // [OHEM_BINS]
    const int H = ay.n_out, W = ax.n_out, h = ay.n_in, w = ax.n_in;
    const int tid = threadIdx.x, b = blockIdx.z;
    const int xa = blockIdx.x * GDL_XT, xb = min(W, xa + GDL_XT);
    const int ya = blockIdx.y * rows, yb = min(H, ya + rows);
    for (int e = tid; e < OHEM_BINS; e += 256) lh[e] = 0u;
    int cbase, clast, unused;
    float lx = 0.f;
    ax.src(xa, cbase, unused, lx);
    ax.src(xb - 1, unused, clast, lx);
    const int ncol = min(clast - cbase + 1, ncol_max);
    const int x = xa + tid;
    int x0 = cbase, x1 = cbase;
    if (x < xb) ax.src(x, x0, x1, lx);
    unsigned nvalid = 0u, bad = 0u;
    for (int y = ya; y < yb; ++y) {
        int y0, y1;
        float ly;
        ay.src(y, y0, y1, ly);
        const float* row0 = low + (((long)b * h + y0) * w + cbase) * K;
        const float* row1 = low + (((long)b * h + y1) * w + cbase) * K;
        for (int e = tid; e < ncol * K; e += 256) vrow[e] = (1.f - ly) * row0[e] + ly * row1[e];
        __syncthreads();
        if (x < xb) {
            const long pix = ((long)b * H + y) * W + x;
            const long lab = labels[pix];
            float q = OHEM_SENTINEL, nll = 0.f;
            if (lab != ignore_index && lab >= 0 && lab < K) {
                const float* c0 = vrow + (x0 - cbase) * K;
                const float* c1 = vrow + (x1 - cbase) * K;
                float v[KR];
                float mx = -3.0e38f;
#pragma unroll
                for (int k = 0; k < KR; ++k) {
                    if (k < K) {
                        v[k] = (1.f - lx) * c0[k] + lx * c1[k];
                        mx = fmaxf(mx, v[k]);
                    }
                }
                float se = 0.f, picked = 0.f, ey = 0.f;      // the loss term from picked = z_y - max before the exponential, as upce_pass1_kernel: finite when q underflows
#pragma unroll
                for (int k = 0; k < KR; ++k) {
                    if (k < K) {
                        if (k == lab) picked = v[k] - mx;
                        v[k] = __expf(v[k] - mx);
                        if (k == lab) ey = v[k];
                        se += v[k];
                    }
                }
                q = fminf(ey * (1.f / se), 1.f);
                nll = __logf(se) - picked;
                nvalid += 1u;
                atomicAdd(&lh[__float_as_uint(q) >> 21], 1u);
            } else if (lab != ignore_index) {
                bad += 1u;
            }
            qout[pix] = q;
            nllout[pix] = nll;
        }
        __syncthreads();          // the next row overwrites vrow
    }
    nvalid = wave_sum(nvalid);
    bad = wave_sum(bad);
    if ((tid & 63) == 0) {
        if (nvalid) atomicAdd(&state[OHEM_NVALID], nvalid);
        if (bad) atomicAdd(&state[OHEM_BAD], bad);
    }
    for (int e = tid; e < OHEM_BINS; e += 256) {
        const unsigned c = lh[e];
        if (c) atomicAdd(&hist[e], c);
    }
}

// One workgroup.  level 0 / 1 / 2 looks at bits 31..21 / 20..10 / 9..0 (2048 / 2048 / 1024 bins).  rank = 1-based rank of the wanted value among the
// values that share the prefix so far (level 0: k = min(kmin, n valid)); rank 0 (no valid pixel) picks bin 0 at every level, so t = thresh.
__global__ __launch_bounds__(256) void ohem_scan_kernel(const unsigned* __restrict__ hist_all, unsigned* __restrict__ state, int level, unsigned kmin,
                                                        float thresh) {
    __shared__ unsigned sc[256];
    const int tid = threadIdx.x;
    const int per = level == 2 ? 4 : 8, width = level == 2 ? 10 : 11;
    const unsigned* hist = hist_all + level * OHEM_BINS;
    const unsigned rank = level == 0 ? min(kmin, state[OHEM_NVALID]) : state[OHEM_RANK];
    const unsigned prefix = level == 0 ? 0u : state[OHEM_PREFIX];
    unsigned c[8], sum = 0u;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        c[i] = i < per ? hist[tid * per + i] : 0u;
        sum += c[i];
    }
    sc[tid] = sum;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {          // inclusive scan of the 256 thread sums
        const unsigned v = tid >= d ? sc[tid - d] : 0u;
        __syncthreads();
        sc[tid] += v;
        __syncthreads();
    }
    const unsigned incl = sc[tid], excl = incl - sum;
    const bool mine = rank > 0u ? (excl < rank && rank <= incl) : tid == 0;          // exactly one thread
    if (mine) {
        unsigned cum = excl;
        int bucket = tid * per;
        if (rank > 0u) {
            bool found = false;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (i < per && !found) {
                    if (cum + c[i] >= rank) {
                        found = true;
                        bucket = tid * per + i;
                    } else {
                        cum += c[i];
                    }
                }
            }
        }
        const unsigned np = (prefix << width) | (unsigned)bucket;
        state[OHEM_PREFIX] = np;
        state[OHEM_RANK] = rank > 0u ? rank - cum : 0u;
        if (level == 2) state[OHEM_T] = __float_as_uint(fmaxf(thresh, __uint_as_float(np)));
    }
}

// Histogram of the next bit field of the values whose higher bits equal the prefix chosen so far.
__global__ __launch_bounds__(256) void ohem_hist_kernel(const unsigned* __restrict__ qbits, int n, unsigned* __restrict__ hist_all,
                                                        const unsigned* __restrict__ state, int level) {
    __shared__ unsigned lh[OHEM_BINS];
    const int tid = threadIdx.x;
    const int hi = level == 1 ? 21 : 10, lo = level == 1 ? 10 : 0;
    const unsigned mask = level == 1 ? 2047u : 1023u;
    const unsigned prefix = state[OHEM_PREFIX];
    for (int e = tid; e < OHEM_BINS; e += 256) lh[e] = 0u;
    __syncthreads();
    for (long i = (long)blockIdx.x * 256 + tid; i < n; i += (long)gridDim.x * 256) {
        const unsigned u = qbits[i];
        if ((u >> hi) == prefix) atomicAdd(&lh[(u >> lo) & mask], 1u);
    }
    __syncthreads();
    unsigned* hist = hist_all + level * OHEM_BINS;
    for (int e = tid; e < OHEM_BINS; e += 256) {
        const unsigned c = lh[e];
        if (c) atomicAdd(&hist[e], c);
    }
}

// partial: [workgroup][2] words - the sum of -log q over the kept pixels (float), their count (unsigned).  A thread adds its pixels in ascending order,
// the wave by butterfly, the four waves in order.
__global__ __launch_bounds__(256) void ohem_loss_kernel(const float* __restrict__ q, const float* __restrict__ nll, int n, const unsigned* __restrict__ state,
                                                        unsigned* __restrict__ partial) {
    __shared__ float rs[4];
    __shared__ unsigned rc[4];
    const int tid = threadIdx.x;
    const float t = __uint_as_float(state[OHEM_T]);
    float s = 0.f;
    unsigned c = 0u;
    for (long i = (long)blockIdx.x * 256 + tid; i < n; i += (long)gridDim.x * 256) {
        if (q[i] <= t) {
            s += nll[i];
            c += 1u;
        }
    }
    s = wave_sum(s);
    c = wave_sum(c);
    if ((tid & 63) == 0) {
        rs[tid >> 6] = s;
        rc[tid >> 6] = c;
    }
    __syncthreads();
    if (tid == 0) {
        partial[2 * blockIdx.x] = __float_as_uint(((rs[0] + rs[1]) + rs[2]) + rs[3]);
        partial[2 * blockIdx.x + 1] = ((rc[0] + rc[1]) + rc[2]) + rc[3];
    }
}

// One workgroup: the partial rows in fp64 / integers in a fixed order, then loss_out = loss, n_kept, out-of-range labels, t.
__global__ __launch_bounds__(256) void ohem_finalize_kernel(const unsigned* __restrict__ partial, int nwg, const unsigned* __restrict__ state,
                                                            float* __restrict__ loss_out) {
    __shared__ double rs[4];
    __shared__ unsigned rc[4];
    const int tid = threadIdx.x;
    double s = 0.0;
    unsigned c = 0u;
    for (int i = tid; i < nwg; i += 256) {
        s += (double)__uint_as_float(partial[2 * i]);
        c += partial[2 * i + 1];
    }
    s = wave_sum(s);
    c = wave_sum(c);
    if ((tid & 63) == 0) {
        rs[tid >> 6] = s;
        rc[tid >> 6] = c;
    }
    __syncthreads();
    if (tid == 0) {
        const double tot = ((rs[0] + rs[1]) + rs[2]) + rs[3];
        const unsigned kept = ((rc[0] + rc[1]) + rc[2]) + rc[3];
        loss_out[0] = (float)(tot / (double)kept);          // 0 / 0 = nan when no pixel is valid, as the other heads
        loss_out[1] = (float)kept;                          // exact: B H W < 2^24
        loss_out[2] = (float)state[OHEM_BAD];
        loss_out[3] = __uint_as_float(state[OHEM_T]);
    }
}

// gdl_grad_kernel's tiling with d = kept (softmax - onehot); kept is read from the stored q (the sentinel of a pixel that is not valid lies above any t),
// and a pixel that is not kept costs neither a label read nor a softmax.
template <int KT>
__global__ __launch_bounds__(256) void ohem_grad_kernel(const float* __restrict__ low, const int64_t* __restrict__ labels, const float* __restrict__ q,
                                                        const unsigned* __restrict__ state, float* __restrict__ tmp, int Krt, Axis ay, Axis ax, int npx_max,
                                                        int jt_cols) {
    const int K = KT > 0 ? KT : Krt;
    constexpr int KR = KT > 0 ? KT : KMAX;
    extern __shared__ __attribute__((aligned(16))) float sh[];
    float* dbuf = sh;                                           // [npx_max][K]
    float* lam = sh + (long)npx_max * K;                        // [npx_max]  lambda_x
    int* pstart = reinterpret_cast<int*>(lam + npx_max);        // [JT+3] first pixel (relative to xa) whose x0 >= j0 - 1 + q
    float* vrow = reinterpret_cast<float*>(pstart + JT + 4);    // [JT+2][K] low-res row already interpolated along y
    const int H = ay.n_out, W = ax.n_out, w = ax.n_in;
    const int jt = blockIdx.x, y = blockIdx.y, b = blockIdx.z;
    const int j0 = jt * jt_cols, j1 = min(w, j0 + jt_cols);
    const int xa = ax.first_with_i0_ge(j0 - 1), xb = ax.first_with_i0_ge(j1);   // pixels with x0 in [j0-1, j1-1]
    const int npx = min(xb - xa, npx_max);
    int cbase;
    tile_stage(low, K, ay, ax, b, y, j0, j1, xa, pstart, vrow, cbase);
    __syncthreads();
    const float t = __uint_as_float(state[OHEM_T]);
    for (int px = threadIdx.x; px < npx; px += 256) {
        const int x = xa + px;
        int x0, x1;
        float lx;
        ax.src(x, x0, x1, lx);
        lam[px] = lx;
        const long pix = ((long)b * H + y) * W + x;
        float* d = dbuf + (long)px * K;
        if (!(q[pix] <= t)) {
            for (int k = 0; k < K; ++k) d[k] = 0.f;
            continue;
        }
        const long lab = labels[pix];
        const float* c0 = vrow + (x0 - cbase) * K;
        const float* c1 = vrow + (x1 - cbase) * K;
        float v[KR];
        float mx = -3.0e38f;
#pragma unroll
        for (int k = 0; k < KR; ++k) {
            if (k < K) {
                v[k] = (1.f - lx) * c0[k] + lx * c1[k];
                mx = fmaxf(mx, v[k]);
            }
        }
        float se = 0.f;
#pragma unroll
        for (int k = 0; k < KR; ++k) {
            if (k < K) {
                v[k] = __expf(v[k] - mx);
                se += v[k];
            }
        }
        const float rse = 1.f / se;
#pragma unroll
        for (int k = 0; k < KR; ++k) {
            if (k < K) d[k] = v[k] * rse - (k == lab ? 1.f : 0.f);
        }
    }
    __syncthreads();
    tile_gather_x(dbuf, lam, pstart, tmp + ((long)b * H + y) * w * K, K, j0, j1, w, npx);
}

struct OhemLayout {
    size_t q, nll, hist, partial, tmp, total;
};
inline OhemLayout ohem_layout(int B, int w, int K, int H, int W) {
    OhemLayout l;
    const size_t n = (size_t)B * H * W;
    l.q = 0;
    l.nll = l.q + up256(n * sizeof(float));
    l.hist = l.nll + up256(n * sizeof(float));
    l.partial = l.hist + up256((3 * OHEM_BINS + OHEM_STATE) * sizeof(unsigned));
    l.tmp = l.partial + up256((size_t)OHEM_WGS * 2 * sizeof(unsigned));
    l.total = l.tmp + (size_t)B * H * w * K * sizeof(float);
    return l;
}
}  // namespace

extern "C" size_t mi_upsample_ce_ohem_workspace(int B, int h, int w, int K, int H, int W) {
    if (B <= 0 || h <= 0 || w <= 0 || K <= 0 || H <= 0 || W <= 0) return 0;
    return ohem_layout(B, w, K, H, W).total;
}

extern "C" int mi_upsample_ce_ohem(const float* low, const int64_t* labels, float* loss_out, float* dlow, float* prob, int B, int h, int w, int K, int H,
                                   int W, int ignore_index, float thresh, int64_t min_kept, float grad_scale, int align_corners, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    MI_REQUIRE(low && labels && loss_out && workspace, "mi_upsample_ce_ohem: null operand");
    MI_REQUIRE(B > 0 && h > 0 && w > 0 && H > 0 && W > 0 && K > 0 && K <= KMAX, "mi_upsample_ce_ohem: bad dimension (K <= 32)");
    MI_REQUIRE(H >= h && W >= w, "mi_upsample_ce_ohem: only upsampling (H >= h, W >= w) is supported");
    MI_REQUIRE(H <= 65535 && B <= 65535, "mi_upsample_ce_ohem: grid dimension overflow");
    MI_REQUIRE((long)B * H * W < (1L << 24), "mi_upsample_ce_ohem: B H W must stay below 2^24 (n_kept is reported as a float)");
    MI_REQUIRE(thresh >= 0.f && thresh <= 1.f, "mi_upsample_ce_ohem: thresh outside [0, 1]");          // (a NaN fails both comparisons)
    MI_REQUIRE(min_kept >= 1, "mi_upsample_ce_ohem: min_kept must be at least 1");
    MI_REQUIRE(std::isfinite(grad_scale), "mi_upsample_ce_ohem: grad_scale is not finite");
    if (workspace_bytes < mi_upsample_ce_ohem_workspace(B, h, w, K, H, W)) return mi_set_error(MI_ENOMEM, "mi_upsample_ce_ohem: workspace too small");
    const Axis ay = make_axis(h, H, align_corners), ax = make_axis(w, W, align_corners);
    const OhemLayout lay = ohem_layout(B, w, K, H, W);
    const GdlPlan pl = gdl_plan(B, H, W);
    char* ws = (char*)workspace;
    float* q = (float*)(ws + lay.q);
    float* nll = (float*)(ws + lay.nll);
    unsigned* hist = (unsigned*)(ws + lay.hist);
    unsigned* state = hist + 3 * OHEM_BINS;
    unsigned* partial = (unsigned*)(ws + lay.partial);
    float* tmp = (float*)(ws + lay.tmp);
    const int n = B * H * W;
    const unsigned kmin = (unsigned)(min_kept < (int64_t)(1 << 24) ? min_kept : (int64_t)(1 << 24));          // k = min(min_kept, n) and n < 2^24
    const int ncol_max = w < GDL_XT + 2 ? w : GDL_XT + 2;
    const size_t lds1 = ((size_t)ncol_max * K + OHEM_BINS) * 4;          // <= 41 KB
    const int jt_cols = pick_jt(w, W);
    const int npx_max = pass1_npx_max(ax, jt_cols);
    const size_t lds3 = (size_t)npx_max * K * 4 + (size_t)npx_max * 4 + (JT + 4) * 4 + (size_t)(JT + 2) * K * 4;
    MI_REQUIRE(!dlow || lds3 <= 160 * 1024, "mi_upsample_ce_ohem: upsample factor too large for one LDS tile (%zu B)", lds3);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(hist, 0, (3 * OHEM_BINS + OHEM_STATE) * sizeof(unsigned), st) != hipSuccess) return mi_set_error(MI_EHIP, "mi_upsample_ce_ohem: memset");
    const dim3 g1(pl.tiles_x, pl.row_groups, B);
    if (K == 19)
        hipLaunchKernelGGL(ohem_prob_kernel<19>, g1, dim3(256), lds1, st, low, labels, q, nll, hist, state, K, ay, ax, ignore_index, pl.rows, ncol_max);
    else
        hipLaunchKernelGGL(ohem_prob_kernel<0>, g1, dim3(256), lds1, st, low, labels, q, nll, hist, state, K, ay, ax, ignore_index, pl.rows, ncol_max);
    MI_CHECK_LAUNCH("mi_upsample_ce_ohem probability");
    const unsigned nwg = nblk(n, 256) < (unsigned)OHEM_WGS ? nblk(n, 256) : (unsigned)OHEM_WGS;
    for (int level = 0; level < 3; ++level) {
        if (level > 0) {
            hipLaunchKernelGGL(ohem_hist_kernel, dim3(nwg), dim3(256), 0, st, (const unsigned*)q, n, hist, (const unsigned*)state, level);
            MI_CHECK_LAUNCH("mi_upsample_ce_ohem histogram");
        }
        hipLaunchKernelGGL(ohem_scan_kernel, dim3(1), dim3(256), 0, st, (const unsigned*)hist, state, level, kmin, thresh);
        MI_CHECK_LAUNCH("mi_upsample_ce_ohem scan");
    }
    hipLaunchKernelGGL(ohem_loss_kernel, dim3(nwg), dim3(256), 0, st, (const float*)q, (const float*)nll, n, (const unsigned*)state, partial);
    MI_CHECK_LAUNCH("mi_upsample_ce_ohem loss");
    hipLaunchKernelGGL(ohem_finalize_kernel, dim3(1), dim3(256), 0, st, (const unsigned*)partial, (int)nwg, (const unsigned*)state, loss_out);
    MI_CHECK_LAUNCH("mi_upsample_ce_ohem finalize");
    if (dlow) {
        static std::atomic<uint64_t> lds_set[2];
        mi_allow_dynamic_lds((const void*)ohem_grad_kernel<19>, MI_LDS_MAX, lds_set[0]);
        mi_allow_dynamic_lds((const void*)ohem_grad_kernel<0>, MI_LDS_MAX, lds_set[1]);
        const int tiles = (w + jt_cols - 1) / jt_cols;
        if (K == 19)
            hipLaunchKernelGGL(ohem_grad_kernel<19>, dim3(tiles, H, B), dim3(256), lds3, st, low, labels, (const float*)q, (const unsigned*)state, tmp, K, ay, ax,
                               npx_max, jt_cols);
        else
            hipLaunchKernelGGL(ohem_grad_kernel<0>, dim3(tiles, H, B), dim3(256), lds3, st, low, labels, (const float*)q, (const unsigned*)state, tmp, K, ay, ax,
                               npx_max, jt_cols);
        MI_CHECK_LAUNCH("mi_upsample_ce_ohem gradient");
        hipLaunchKernelGGL(wce_pass2_kernel, dim3(nblk((long)B * h * w * K, 256)), dim3(256), 0, st, (const float*)tmp, (const float*)loss_out, dlow, B, K, ay, w,
                           grad_scale);
        MI_CHECK_LAUNCH("mi_upsample_ce_ohem gradient rows");
    }
    if (prob && hipMemcpyAsync(prob, q, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
        return mi_set_error(MI_EHIP, "mi_upsample_ce_ohem: copy of q");
    return MI_OK;
}

extern "C" int mi_upsample_softmax(const float* low, float* probs, uint8_t* pred, int B, int h, int w, int K, int H, int W, void* stream) {
    MI_REQUIRE(low && probs && B > 0 && h > 0 && w > 0 && H > 0 && W > 0 && K > 0 && K <= KMAX, "mi_upsample_softmax: bad argument (K <= 32)");
    hipLaunchKernelGGL(upsample_softmax_kernel, dim3(nblk((long)B * H * W, 256)), dim3(256), 0, (hipStream_t)stream, low, probs, pred, B, K,
                       make_axis(h, H), make_axis(w, W));
    MI_CHECK_LAUNCH("mi_upsample_softmax");
    return MI_OK;
}

extern "C" int mi_upsample_softmax_multi(const MiProbSource* src, int n, float* probs, int K, int H, int W, float div_a, float div_b,
                                         void* stream) {
    MI_REQUIRE(src && probs, "mi_upsample_softmax_multi: null operand");
    MI_REQUIRE(n >= 1 && n <= MAX_PROB_SRC, "mi_upsample_softmax_multi: 1 <= n <= 16 sources");
    MI_REQUIRE(K > 0 && K <= KMAX && H > 0 && W > 0, "mi_upsample_softmax_multi: bad dimension (K <= 32)");
    MI_REQUIRE(div_a != 0.f && div_b != 0.f, "mi_upsample_softmax_multi: zero divisor");
    ProbSrcs srcs;
    for (int i = 0; i < MAX_PROB_SRC; ++i) {
        const MiProbSource& m = src[i < n ? i : 0];       // unused slots repeat source 0: never read, never uninitialised
        MI_REQUIRE(m.low && m.h > 0 && m.w > 0, "mi_upsample_softmax_multi: bad source");
        srcs.s[i] = ProbSrc{m.low, make_axis(m.h, H), make_axis(m.w, W), m.mirror != 0};
    }
    const bool wide = W % 2 == 0 && (reinterpret_cast<uintptr_t>(probs) & 7) == 0;
    const unsigned nb = nblk((long)H * (wide ? W / 2 : W), 256);
#define MI_LAUNCH_MULTI(KT, P) \
    hipLaunchKernelGGL((upsample_softmax_multi_kernel<KT, P>), dim3(nb), dim3(256), 0, (hipStream_t)stream, srcs, n, probs, K, H, W, div_a, div_b)
    if (K == 19) {
        if (wide) MI_LAUNCH_MULTI(19, 2); else MI_LAUNCH_MULTI(19, 1);
    } else {
        if (wide) MI_LAUNCH_MULTI(0, 2); else MI_LAUNCH_MULTI(0, 1);
    }
#undef MI_LAUNCH_MULTI
    MI_CHECK_LAUNCH("mi_upsample_softmax_multi");
    return MI_OK;
}

extern "C" int mi_upsample_predict_score(const MiProbSource* src, int n, int K, int H, int W, float div_a, float div_b, const int64_t* labels,
                                         int ignore_index, float threshold, uint8_t* pred, uint8_t* pseudo, int64_t* counts, void* stream) {
    MI_REQUIRE(src && pred, "mi_upsample_predict_score: null operand");
    MI_REQUIRE(n >= 1 && n <= MAX_PROB_SRC, "mi_upsample_predict_score: 1 <= n <= 16 sources");
    MI_REQUIRE(K > 0 && K <= KMAX && H > 0 && W > 0, "mi_upsample_predict_score: bad dimension (K <= 32)");
    MI_REQUIRE(div_a != 0.f && div_b != 0.f, "mi_upsample_predict_score: zero divisor");
    MI_REQUIRE((labels != nullptr) == (counts != nullptr), "mi_upsample_predict_score: labels and counts go together");
    MI_REQUIRE(ignore_index < 0 || ignore_index >= K, "mi_upsample_predict_score: ignore_index inside [0, K)");
    MI_REQUIRE(threshold >= 0.f && threshold <= 1.f, "mi_upsample_predict_score: threshold outside [0, 1]");
    ProbSrcs srcs;
    for (int i = 0; i < MAX_PROB_SRC; ++i) {
        const MiProbSource& m = src[i < n ? i : 0];       // unused slots repeat source 0: never read, never uninitialised
        MI_REQUIRE(m.low && m.h > 0 && m.w > 0, "mi_upsample_predict_score: bad source");
        srcs.s[i] = ProbSrc{m.low, make_axis(m.h, H), make_axis(m.w, W), m.mirror != 0};
    }
    const bool wide = W % 2 == 0 && (reinterpret_cast<uintptr_t>(pred) & 1) == 0 && (reinterpret_cast<uintptr_t>(pseudo) & 1) == 0 &&
                      (reinterpret_cast<uintptr_t>(labels) & 15) == 0;
    const unsigned nb = nblk((long)H * (wide ? W / 2 : W), 256);
#define MI_LAUNCH_SCORE(KT, P)                                                                                                                 \
    hipLaunchKernelGGL((upsample_predict_score_kernel<KT, P>), dim3(nb), dim3(256), 0, (hipStream_t)stream, srcs, n, K, H, W, div_a, div_b, \
                       reinterpret_cast<const long long*>(labels), ignore_index, threshold, pred, pseudo, reinterpret_cast<unsigned long long*>(counts))
    if (K == 19) {
        if (wide) MI_LAUNCH_SCORE(19, 2); else MI_LAUNCH_SCORE(19, 1);
    } else {
        if (wide) MI_LAUNCH_SCORE(0, 2); else MI_LAUNCH_SCORE(0, 1);
    }
#undef MI_LAUNCH_SCORE
    MI_CHECK_LAUNCH("mi_upsample_predict_score");
    return MI_OK;
}

extern "C" int mi_image_resize_ac(const float* x, float* out, int B, int C, int H, int W, int Ho, int Wo, int with_mirror, void* stream) {
    MI_REQUIRE(x && out && B > 0 && C > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0, "mi_image_resize_ac: bad argument");
    hipLaunchKernelGGL(image_resize_ac_kernel, dim3(nblk((long)B * C * Ho * Wo, 256)), dim3(256), 0, (hipStream_t)stream, x, out, B, C,
                       make_axis(H, Ho), make_axis(W, Wo), with_mirror != 0);
    MI_CHECK_LAUNCH("mi_image_resize_ac");
    return MI_OK;
}
