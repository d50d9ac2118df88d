// Kernels of the FADA adversarial step: conv bias gradient, fused bilinear upsample + soft-label
// cross-entropy with on-the-fly soft labels, Adam.  References: core/combos/aspp_fada.py:80-127,
// core/utils/utility.py:172-177 (soft_label_cross_entropy), core/adapters/fada_adapter.py:24 (Adam betas .9/.99).
// fp32 arithmetic, fixed summation orders (bitwise reproducible), HBM-bound.
#include "upsample_common.h"      // Axis, the x-tile staging / gather of upce_pass1_kernel (KMAX, JT), nblk, pass1_npx_max

namespace {

__device__ __forceinline__ void block_sum(float& a, float* red) {
    const int t = threadIdx.x;
    red[t] = a;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    a = red[0];
    __syncthreads();
}

// pass 1: workgroup = (b, y, tile of JT low-res columns).  Per high-res pixel (once): soft labels from the segmentation logits,
// log-softmax of the 2K discriminator logits, loss term, d = S*softmax(z) - placed(soft) into LDS; then gather along x.
// KT > 0: compile-time class count (19: exact-length unrolled loops, soft labels indexed statically); KT == 0: runtime K.
template <int KT>
__global__ __launch_bounds__(256) void softce_pass1_kernel(const float* __restrict__ seg, float inv_t, float clip, const float* __restrict__ dl,
                                                           int ldD, int domain, float* __restrict__ partial, float* __restrict__ tmp, int B,
                                                           int Krt, Axis ay, Axis ax, int npx_max) {
    extern __shared__ __attribute__((aligned(16))) float sh[];
    const int K = KT > 0 ? KT : Krt;
    constexpr int KR = KT > 0 ? KT : KMAX;
    const int K2 = 2 * K;
    float* dbuf = sh;                                   // [npx_max][K2]
    float* red = dbuf + (long)npx_max * K2;             // [256]
    int* pstart = reinterpret_cast<int*>(red + 256);    // [JT+3] first pixel (relative to xa) whose x0 >= j0 - 1 + q
    float* srow = red + 256 + JT + 4;                   // [JT+2][K]   seg logits interpolated along y
    float* drow = srow + (JT + 2) * K;                  // [JT+2][K2]  discriminator logits interpolated along y
    float* lam = drow + (JT + 2) * K2;                  // [npx_max]   last: every region before it starts at an even offset (8-byte LDS accesses)
    const int H = ay.n_out, h = ay.n_in, w = ax.n_in;
    const int jt = blockIdx.x, y = blockIdx.y, b = blockIdx.z;
    const int j0 = jt * JT, j1 = min(w, j0 + JT);
    const int xa = ax.first_with_i0_ge(j0 - 1), xb = ax.first_with_i0_ge(j1);
    const int npx = xb - xa;
    int y0, y1;
    float ly;
    ay.src(y, y0, y1, ly);
    const int cbase = max(j0 - 1, 0), ncol = min(j1, w - 1) - cbase + 1;
    if (threadIdx.x < j1 - j0 + 2) pstart[threadIdx.x] = ax.first_with_i0_ge(j0 - 1 + (int)threadIdx.x) - xa;
    for (int e = threadIdx.x; e < ncol * K; e += 256) {
        const int c = e / K, k = e - c * K;
        const long o0 = (((long)b * h + y0) * w + cbase + c) * K + k, o1 = (((long)b * h + y1) * w + cbase + c) * K + k;
        srow[e] = (1.f - ly) * seg[o0] + ly * seg[o1];
    }
    for (int e = threadIdx.x; e < ncol * K2; e += 256) {
        const int c = e / K2, k = e - c * K2;
        const long o0 = (((long)b * h + y0) * w + cbase + c) * ldD + k, o1 = (((long)b * h + y1) * w + cbase + c) * ldD + k;
        drow[e] = (1.f - ly) * dl[o0] + ly * dl[o1];
    }
    __syncthreads();
    float loss = 0.f;
    for (int px = threadIdx.x; px < npx; px += 256) {
        const int x = xa + px;
        int x0, x1;
        float lx;
        ax.src(x, x0, x1, lx);
        lam[px] = lx;
        const float* s0 = srow + (x0 - cbase) * K;
        const float* s1 = srow + (x1 - cbase) * K;
        const float* z0 = drow + (x0 - cbase) * K2;
        const float* z1 = drow + (x1 - cbase) * K2;
        // soft labels: softmax(seg / T), clipped (aspp_fada.py:91-103)
        float soft[KR];
        float mx = -3.0e38f;
#pragma unroll
        for (int k = 0; k < KR; ++k)
            if (k < K) {
                soft[k] = ((1.f - lx) * s0[k] + lx * s1[k]) * inv_t;
                mx = fmaxf(mx, soft[k]);
            }
        float se = 0.f;
#pragma unroll
        for (int k = 0; k < KR; ++k)
            if (k < K) {
                soft[k] = __expf(soft[k] - mx);
                se += soft[k];
            }
        float S = 0.f;
        const float rse = 1.f / se;
#pragma unroll
        for (int k = 0; k < KR; ++k)
            if (k < K) {
                soft[k] = fminf(soft[k] * rse, clip);
                S += soft[k];
            }
        // discriminator log-softmax over 2K channels (two sweeps over LDS instead of 2K registers)
        float zm = -3.0e38f;
        for (int k = 0; k < K2; ++k) zm = fmaxf(zm, (1.f - lx) * z0[k] + lx * z1[k]);
        float ze = 0.f;
        for (int k = 0; k < K2; ++k) ze += __expf((1.f - lx) * z0[k] + lx * z1[k] - zm);
        const float lse = zm + __logf(ze), rze = 1.f / ze;
        float* d = dbuf + (long)px * K2;
        float l = 0.f;
        if (KT > 0) {                     // channel k = half*K + q carries soft[q] when half == domain, else 0: static indices
#pragma unroll
            for (int half = 0; half < 2; ++half)
#pragma unroll
                for (int q = 0; q < KR; ++q) {
                    const int k = half * KR + q;
                    const float z = (1.f - lx) * z0[k] + lx * z1[k];
                    const float placed = (half == domain) ? soft[q] : 0.f;
                    l -= placed * (z - lse);
                    d[k] = S * __expf(z - zm) * rze - placed;
                }
        } else {
            for (int k = 0; k < K2; ++k) {
                const float z = (1.f - lx) * z0[k] + lx * z1[k];
                float placed = 0.f;
                const int c = k - domain * K;
#pragma unroll
                for (int q = 0; q < KMAX; ++q)
                    if (q == c) placed = soft[q];
                l -= placed * (z - lse);
                d[k] = S * __expf(z - zm) * rze - placed;
            }
        }
        if (x0 >= j0) loss += l;          // the tile that owns x0 accounts for the pixel's loss
    }
    __syncthreads();
    if (tmp) tile_gather_x(dbuf, lam, pstart, tmp + ((long)b * H + y) * w * K2, K2, j0, j1, w, npx);
    block_sum(loss, red);
    if (threadIdx.x == 0) partial[((long)b * H + y) * gridDim.x + jt] = loss;
}

__global__ void softce_finalize_kernel(const float* __restrict__ partial, int n, float count, float* __restrict__ loss_out) {
    __shared__ float red[256];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += partial[i];
    block_sum(s, red);
    if (threadIdx.x == 0) {
        loss_out[0] = s / count;
        loss_out[1] = count;
    }
}

// pass 2: dd_low[b][i][j][k] = grad_scale / count * sum_y wy(y,i) tmp[b][y][j][k]
__global__ void softce_pass2_kernel(const float* __restrict__ tmp, float* __restrict__ dd, int B, int K2, int ldD, Axis ay, int w,
                                    float scale) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int H = ay.n_out, h = ay.n_in;
    const long per_row = (long)w * K2;
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
    const int j = (int)(jk / K2), k = (int)(jk - (long)j * K2);
    dd[(((long)b * h + i) * w + j) * ldD + k] = s * scale;
}

// Two-grid variant (GaldFada: the segmentation logits at 1/4 resolution, align_corners=False, the discriminator's at 1/32, align_corners=True;
// gald_fada.py:96-121).  Workgroup = (b, y, tile of jt discriminator columns).  The tile's high-res pixels go through in batches of NB, one per
// thread: soft labels straight from the four segmentation corners (global / L2: no LDS that grows with that grid's ratio), log-softmax of the
// 2K discriminator logits from a y-interpolated row of the tile's columns, loss term, d = S*softmax(z) - placed(soft) into LDS; after each batch
// every (column, channel) item of the tile adds the batch's pixels in pixel order (registers, fixed order: bitwise reproducible).  LDS is
// NB * 2K + (jt + 2) * 2K floats whatever the upsample factors.
constexpr int NB = 256;        // pixels per batch (= threads)
constexpr int JT2 = 32;        // most discriminator columns per tile
constexpr int ITEMS = 8;       // (column, channel) items per thread: jt * 2K <= NB * ITEMS

template <int KT>
__global__ __launch_bounds__(256) void softce2_pass1_kernel(const float* __restrict__ seg, Axis sy, Axis sx, float inv_t, float clip,
                                                            const float* __restrict__ dl, int ldD, int domain, float* __restrict__ partial,
                                                            float* __restrict__ tmp, int Krt, Axis ay, Axis ax, int jt_cols) {
    extern __shared__ __attribute__((aligned(16))) float sh[];
    const int K = KT > 0 ? KT : Krt;
    constexpr int KR = KT > 0 ? KT : KMAX;
    const int K2 = 2 * K;
    float* dbuf = sh;                                   // [NB][K2]
    float* lam = dbuf + NB * K2;                        // [NB]
    float* red = lam + NB;                              // [256]
    int* pstart = reinterpret_cast<int*>(red + 256);    // [JT2+3] first pixel (relative to xa) whose x0 >= j0 - 1 + q
    float* drow = red + 256 + JT2 + 4;                  // [JT2+2][K2]  discriminator logits interpolated along y
    const int H = ay.n_out, hd = ay.n_in, wd = ax.n_in, hs = sy.n_in, ws = sx.n_in;
    const int jt = blockIdx.x, y = blockIdx.y, b = blockIdx.z;
    const int j0 = jt * jt_cols, j1 = min(wd, j0 + jt_cols);
    const int xa = ax.first_with_i0_ge(j0 - 1), xb = ax.first_with_i0_ge(j1);
    const int npx = xb - xa;
    int y0, y1, t0, t1;
    float ly, lt;
    ay.src(y, y0, y1, ly);
    sy.src(y, t0, t1, lt);
    const float* srow0 = seg + ((long)b * hs + t0) * ws * K;
    const float* srow1 = seg + ((long)b * hs + t1) * ws * K;
    const int cbase = max(j0 - 1, 0), ncol = min(j1, wd - 1) - cbase + 1;
    if (threadIdx.x < j1 - j0 + 2) pstart[threadIdx.x] = ax.first_with_i0_ge(j0 - 1 + (int)threadIdx.x) - xa;
    for (int e = threadIdx.x; e < ncol * K2; e += 256) {
        const int c = e / K2, k = e - c * K2;
        const long o0 = (((long)b * hd + y0) * wd + cbase + c) * ldD + k, o1 = (((long)b * hd + y1) * wd + cbase + c) * ldD + k;
        drow[e] = (1.f - ly) * dl[o0] + ly * dl[o1];
    }
    __syncthreads();
    const int nj = j1 - j0, nitems = nj * K2;
    float acc[ITEMS];
#pragma unroll
    for (int r = 0; r < ITEMS; ++r) acc[r] = 0.f;
    float loss = 0.f;
    for (int pb = 0; pb < npx; pb += NB) {
        const int px = pb + (int)threadIdx.x;
        if (px < npx) {
            const int x = xa + px;
            int x0, x1, u0, u1;
            float lx, lu;
            ax.src(x, x0, x1, lx);
            sx.src(x, u0, u1, lu);
            lam[threadIdx.x] = lx;
            const float* z0 = drow + (x0 - cbase) * K2;
            const float* z1 = drow + (x1 - cbase) * K2;
            // soft labels: softmax(up(seg) / T), clipped (gald_fada.py:96-103); y first, then x (the order of softce_pass1_kernel's rows)
            float soft[KR];
            float mx = -3.0e38f;
#pragma unroll
            for (int k = 0; k < KR; ++k)
                if (k < K) {
                    const float a = (1.f - lt) * srow0[u0 * K + k] + lt * srow1[u0 * K + k];
                    const float c = (1.f - lt) * srow0[u1 * K + k] + lt * srow1[u1 * K + k];
                    soft[k] = ((1.f - lu) * a + lu * c) * inv_t;
                    mx = fmaxf(mx, soft[k]);
                }
            float se = 0.f;
#pragma unroll
            for (int k = 0; k < KR; ++k)
                if (k < K) {
                    soft[k] = __expf(soft[k] - mx);
                    se += soft[k];
                }
            float S = 0.f;
            const float rse = 1.f / se;
#pragma unroll
            for (int k = 0; k < KR; ++k)
                if (k < K) {
                    soft[k] = fminf(soft[k] * rse, clip);
                    S += soft[k];
                }
            float zm = -3.0e38f;
            for (int k = 0; k < K2; ++k) zm = fmaxf(zm, (1.f - lx) * z0[k] + lx * z1[k]);
            float ze = 0.f;
            for (int k = 0; k < K2; ++k) ze += __expf((1.f - lx) * z0[k] + lx * z1[k] - zm);
            const float lse = zm + __logf(ze), rze = 1.f / ze;
            float* d = dbuf + threadIdx.x * K2;
            float l = 0.f;
            if (KT > 0) {
#pragma unroll
                for (int half = 0; half < 2; ++half)
#pragma unroll
                    for (int q = 0; q < KR; ++q) {
                        const int k = half * KR + q;
                        const float z = (1.f - lx) * z0[k] + lx * z1[k];
                        const float placed = (half == domain) ? soft[q] : 0.f;
                        l -= placed * (z - lse);
                        d[k] = S * __expf(z - zm) * rze - placed;
                    }
            } else {
                for (int k = 0; k < K2; ++k) {
                    const float z = (1.f - lx) * z0[k] + lx * z1[k];
                    float placed = 0.f;
                    const int c = k - domain * K;
#pragma unroll
                    for (int q = 0; q < KMAX; ++q)
                        if (q == c) placed = soft[q];
                    l -= placed * (z - lse);
                    d[k] = S * __expf(z - zm) * rze - placed;
                }
            }
            if (x0 >= j0) loss += l;      // the tile that owns x0 accounts for the pixel's loss
        }
        if (tmp) {
            __syncthreads();
            const int pe = min(npx, pb + NB);
#pragma unroll
            for (int r = 0; r < ITEMS; ++r) {
                const int item = (int)threadIdx.x + r * NB;
                if (item < nitems) {
                    const int jj = item / K2, k = item - jj * K2;
                    const bool edge = j0 + jj == wd - 1;
                    // pixels with x0 == j-1 contribute lam (as x1), then pixels with x0 == j contribute 1-lam (+ lam at the clamped right edge)
                    const int p0 = max(max(pstart[jj], 0), pb), p1 = min(max(max(pstart[jj + 1], 0), pb), pe);
                    const int p2 = min(pstart[jj + 2], pe);
                    float s = acc[r];
                    for (int p = p0; p < p1; ++p) s += (0.f + lam[p - pb]) * dbuf[(p - pb) * K2 + k];
                    for (int p = max(p1, pb); p < p2; ++p) s += ((1.f - lam[p - pb]) + (edge ? lam[p - pb] : 0.f)) * dbuf[(p - pb) * K2 + k];
                    acc[r] = s;
                }
            }
            __syncthreads();
        }
    }
    if (tmp) {
#pragma unroll
        for (int r = 0; r < ITEMS; ++r) {
            const int item = (int)threadIdx.x + r * NB;
            if (item < nitems) {
                const int jj = item / K2, k = item - jj * K2;
                tmp[(((long)b * H + y) * wd + j0 + jj) * K2 + k] = acc[r];
            }
        }
    }
    block_sum(loss, red);
    if (threadIdx.x == 0) partial[((long)b * H + y) * gridDim.x + jt] = loss;
}

// torch.optim.Adam single-tensor update; CLAMP: the gradient is first clamped to [-clamp, clamp] IN PLACE (core/utils/utils.py:6-16
// clip_gradient, called before optimizer.step() at pranet_trainer.py:59)
template <bool CLAMP>
__global__ void adam_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, size_t n,
                            float step_size, float beta1, float beta2, float inv_sqrt_bc2, float eps, float clamp) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        float gi = g[i];
        if (CLAMP) {
            gi = fminf(fmaxf(gi, -clamp), clamp);
            g[i] = gi;
        }
        const float mi = beta1 * m[i] + (1.f - beta1) * gi;
        const float vi = beta2 * v[i] + (1.f - beta2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        p[i] -= step_size * mi / (sqrtf(vi) * inv_sqrt_bc2 + eps);
    }
}

// The same update with every hyper-parameter read from DEVICE memory (hyper = {lr, beta1, beta2, eps, grad_clamp (<= 0: none), step}): a
// captured HIP graph freezes by-value kernel arguments, and Adam's bias corrections change with the step count on every replay.
__global__ void adam_dev_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, size_t n,
                                const float* __restrict__ hyper) {
    const float lr = hyper[0], beta1 = hyper[1], beta2 = hyper[2], eps = hyper[3], clamp = hyper[4], step = hyper[5];
    const float step_size = (float)((double)lr / (1.0 - pow((double)beta1, (double)step)));
    const float inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow((double)beta2, (double)step)));
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        float gi = g[i];
        if (clamp > 0.f) {
            gi = fminf(fmaxf(gi, -clamp), clamp);
            g[i] = gi;
        }
        const float mi = beta1 * m[i] + (1.f - beta1) * gi;
        const float vi = beta2 * v[i] + (1.f - beta2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        p[i] -= step_size * mi / (sqrtf(vi) * inv_sqrt_bc2 + eps);
    }
}

}  // namespace

extern "C" size_t mi_upsample_softce_workspace(int B, int h, int w, int K, int H, int W) {
    const size_t tiles = (size_t)((w + JT - 1) / JT);
    const size_t partial = (((size_t)B * H * tiles * sizeof(float)) + 255) & ~(size_t)255;
    return partial + (size_t)B * H * w * 2 * K * sizeof(float);
}

extern "C" int mi_upsample_softce(const float* seg_low, float inv_temperature, float clip, const float* d_low, int ldD, int domain,
                                  float* loss_out, float* dd_low, int B, int h, int w, int K, int H, int W, float grad_scale,
                                  void* workspace, size_t workspace_bytes, void* stream) {
    MI_REQUIRE(seg_low && d_low && loss_out && workspace, "mi_upsample_softce: null operand");
    MI_REQUIRE(B > 0 && h > 0 && w > 0 && H >= h && W >= w && K > 0 && K <= KMAX && ldD >= 2 * K, "mi_upsample_softce: bad dimension");
    MI_REQUIRE(domain == 0 || domain == 1, "mi_upsample_softce: domain is 0 (source half) or 1 (target half)");
    MI_REQUIRE(H <= 65535 && B <= 65535, "mi_upsample_softce: grid dimension overflow");
    if (workspace_bytes < mi_upsample_softce_workspace(B, h, w, K, H, W)) return mi_set_error(MI_ENOMEM, "mi_upsample_softce: workspace too small");
    const Axis ay = make_axis(h, H), ax = make_axis(w, W);
    const int tiles = (w + JT - 1) / JT, K2 = 2 * K;
    float* partial = (float*)workspace;
    const size_t poff = (((size_t)B * H * tiles * sizeof(float)) + 255) & ~(size_t)255;
    float* tmp = dd_low ? (float*)((char*)workspace + poff) : nullptr;
    const int npx_max = pass1_npx_max(ax, JT);
    const size_t lds = ((size_t)npx_max * K2 + (size_t)npx_max + 256 + (JT + 4) + (size_t)(JT + 2) * (K + K2)) * 4;
    MI_REQUIRE(lds <= 160 * 1024, "mi_upsample_softce: upsample factor too large for one LDS tile (%zu B)", lds);
    static std::atomic<uint64_t> lds_set[2];
    mi_allow_dynamic_lds((const void*)softce_pass1_kernel<19>, MI_LDS_MAX, lds_set[0]);
    mi_allow_dynamic_lds((const void*)softce_pass1_kernel<0>, MI_LDS_MAX, lds_set[1]);
    if (K == 19)
        hipLaunchKernelGGL(softce_pass1_kernel<19>, dim3(tiles, H, B), dim3(256), lds, (hipStream_t)stream, seg_low, inv_temperature, clip, d_low,
                           ldD, domain, partial, tmp, B, K, ay, ax, npx_max);
    else
        hipLaunchKernelGGL(softce_pass1_kernel<0>, dim3(tiles, H, B), dim3(256), lds, (hipStream_t)stream, seg_low, inv_temperature, clip, d_low,
                           ldD, domain, partial, tmp, B, K, ay, ax, npx_max);
    MI_CHECK_LAUNCH("mi_upsample_softce pass1");
    const float count = (float)B * (float)H * (float)W;
    hipLaunchKernelGGL(softce_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)partial, B * H * tiles, count, loss_out);
    MI_CHECK_LAUNCH("mi_upsample_softce finalize");
    if (dd_low) {
        if (ldD > K2) {
            hipError_t e = hipMemsetAsync(dd_low, 0, (size_t)B * h * w * ldD * sizeof(float), (hipStream_t)stream);
            if (e != hipSuccess) return mi_set_error(MI_EHIP, "mi_upsample_softce: memset: %s", hipGetErrorString(e));
        }
        hipLaunchKernelGGL(softce_pass2_kernel, dim3(nblk((long)B * h * w * K2, 256)), dim3(256), 0, (hipStream_t)stream, (const float*)tmp, dd_low,
                           B, K2, ldD, ay, w, grad_scale / count);
        MI_CHECK_LAUNCH("mi_upsample_softce pass2");
    }
    return MI_OK;
}

// discriminator columns per tile of softce2_pass1_kernel: about NB high-res pixels per tile, within the item budget of a thread
inline int softce2_cols(int wd, int W, int K2) {
    int c = (int)((long)NB * wd / W);
    c = c < 1 ? 1 : c;
    c = c > JT2 ? JT2 : c;
    return c > NB * ITEMS / K2 ? NB * ITEMS / K2 : c;
}

inline size_t softce2_partial_bytes(int B, int wd, int H) { return (((size_t)B * H * wd * sizeof(float)) + 255) & ~(size_t)255; }

extern "C" size_t mi_upsample_softce_2grid_workspace(int B, int hd, int wd, int K, int H, int W) {
    (void)hd;
    (void)W;
    return softce2_partial_bytes(B, wd, H) + (size_t)B * H * wd * 2 * K * sizeof(float);
}

extern "C" int mi_upsample_softce_2grid(const float* seg_low, int hs, int ws, int seg_align_corners, float inv_temperature, float clip,
                                        const float* d_low, int hd, int wd, int ldD, int d_align_corners, int domain, float grad_scale,
                                        float* loss_out, float* dd_low, int B, int K, int H, int W, void* workspace, size_t workspace_bytes,
                                        void* stream) {
    MI_REQUIRE(seg_low && d_low && loss_out && workspace, "mi_upsample_softce_2grid: null operand");
    MI_REQUIRE(K > 0 && K <= KMAX, "mi_upsample_softce_2grid: K = %d, supported 1..%d", K, KMAX);
    MI_REQUIRE(ldD >= 2 * K, "mi_upsample_softce_2grid: ldD = %d < 2K = %d", ldD, 2 * K);
    MI_REQUIRE(domain == 0 || domain == 1, "mi_upsample_softce_2grid: domain is 0 (source half) or 1 (target half), got %d", domain);
    MI_REQUIRE((seg_align_corners == 0 || seg_align_corners == 1) && (d_align_corners == 0 || d_align_corners == 1),
               "mi_upsample_softce_2grid: align_corners flags are 0 or 1");
    MI_REQUIRE(B > 0 && hs > 0 && ws > 0 && hd > 0 && wd > 0 && H >= hs && W >= ws && H >= hd && W >= wd,
               "mi_upsample_softce_2grid: bad dimension (both grids upsample to H x W)");
    MI_REQUIRE(H <= 65535 && B <= 65535, "mi_upsample_softce_2grid: grid dimension overflow");
    MI_REQUIRE(inv_temperature > 0.f && clip > 0.f, "mi_upsample_softce_2grid: inv_temperature and clip must be positive");
    if (workspace_bytes < mi_upsample_softce_2grid_workspace(B, hd, wd, K, H, W))
        return mi_set_error(MI_ENOMEM, "mi_upsample_softce_2grid: workspace too small");
    const Axis ay = make_axis(hd, H, d_align_corners), ax = make_axis(wd, W, d_align_corners);
    const Axis sy = make_axis(hs, H, seg_align_corners), sx = make_axis(ws, W, seg_align_corners);
    const int K2 = 2 * K, jt_cols = softce2_cols(wd, W, K2), tiles = (wd + jt_cols - 1) / jt_cols;
    float* partial = (float*)workspace;
    float* tmp = dd_low ? (float*)((char*)workspace + softce2_partial_bytes(B, wd, H)) : nullptr;
    const size_t lds = ((size_t)NB * K2 + NB + 256 + (JT2 + 4) + (size_t)(JT2 + 2) * K2) * 4;
    static std::atomic<uint64_t> lds_set[2];
    mi_allow_dynamic_lds((const void*)softce2_pass1_kernel<19>, MI_LDS_MAX, lds_set[0]);
    mi_allow_dynamic_lds((const void*)softce2_pass1_kernel<0>, MI_LDS_MAX, lds_set[1]);
    if (K == 19)
        hipLaunchKernelGGL(softce2_pass1_kernel<19>, dim3(tiles, H, B), dim3(256), lds, (hipStream_t)stream, seg_low, sy, sx, inv_temperature, clip,
                           d_low, ldD, domain, partial, tmp, K, ay, ax, jt_cols);
    else
        hipLaunchKernelGGL(softce2_pass1_kernel<0>, dim3(tiles, H, B), dim3(256), lds, (hipStream_t)stream, seg_low, sy, sx, inv_temperature, clip,
                           d_low, ldD, domain, partial, tmp, K, ay, ax, jt_cols);
    MI_CHECK_LAUNCH("mi_upsample_softce_2grid pass1");
    const float count = (float)B * (float)H * (float)W;
    hipLaunchKernelGGL(softce_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)partial, B * H * tiles, count, loss_out);
    MI_CHECK_LAUNCH("mi_upsample_softce_2grid finalize");
    if (dd_low) {
        if (ldD > K2) {
            hipError_t e = hipMemsetAsync(dd_low, 0, (size_t)B * hd * wd * ldD * sizeof(float), (hipStream_t)stream);
            if (e != hipSuccess) return mi_set_error(MI_EHIP, "mi_upsample_softce_2grid: memset: %s", hipGetErrorString(e));
        }
        hipLaunchKernelGGL(softce_pass2_kernel, dim3(nblk((long)B * hd * wd * K2, 256)), dim3(256), 0, (hipStream_t)stream, (const float*)tmp, dd_low,
                           B, K2, ldD, ay, wd, grad_scale / count);
        MI_CHECK_LAUNCH("mi_upsample_softce_2grid pass2");
    }
    return MI_OK;
}

extern "C" int mi_adam_step(float* p, const float* g, float* exp_avg, float* exp_avg_sq, size_t n, float lr, float beta1, float beta2,
                            float eps, int step, void* stream) {
    MI_REQUIRE(p && g && exp_avg && exp_avg_sq && n > 0 && step >= 1, "mi_adam_step: bad argument");
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    size_t blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(adam_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, const_cast<float*>(g), exp_avg, exp_avg_sq, n,
                       (float)(lr / bc1), beta1, beta2, (float)(1.0 / sqrt(bc2)), eps, 0.f);
    MI_CHECK_LAUNCH("mi_adam_step");
    return MI_OK;
}

extern "C" int mi_adam_step_dev(float* p, float* g, float* exp_avg, float* exp_avg_sq, size_t n, const float* hyper, void* stream) {
    MI_REQUIRE(p && g && exp_avg && exp_avg_sq && hyper && n > 0, "mi_adam_step_dev: bad argument");
    size_t blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(adam_dev_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, exp_avg, exp_avg_sq, n, hyper);
    MI_CHECK_LAUNCH("mi_adam_step_dev");
    return MI_OK;
}

extern "C" int mi_adam_step_clamped(float* p, float* g, float* exp_avg, float* exp_avg_sq, size_t n, float lr, float beta1, float beta2,
                                    float eps, int step, float grad_clamp, void* stream) {
    MI_REQUIRE(p && g && exp_avg && exp_avg_sq && n > 0 && step >= 1 && grad_clamp > 0.f, "mi_adam_step_clamped: bad argument");
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    size_t blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(adam_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, exp_avg, exp_avg_sq, n, (float)(lr / bc1),
                       beta1, beta2, (float)(1.0 / sqrt(bc2)), eps, grad_clamp);
    MI_CHECK_LAUNCH("mi_adam_step_clamped");
    return MI_OK;
}
