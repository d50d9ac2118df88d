// Bilinear upsample (align_corners=True), per-pixel softmax cross-entropy with ignore_index, and their fusion with the training losses.
//   F.interpolate(..., mode='bilinear', align_corners=True)   reference core/models/classifiers/aspp/classifier.py:31,
//                                                              core/utils/utility.py:185
//   torch.nn.CrossEntropyLoss(ignore_index=255)               reference core/trainers/aspp_trainer.py:61,91
// All arithmetic fp32 (kept fp32 in bf16 mode too).  HBM-bound: the fused training path reads the
// 1/8-resolution logits (5.7 MB at B=8, 769x769) and labels and never writes the 360 MB [B,19,769,769] tensor.
// Every reduction has a fixed summation order (no float atomics) so results are bitwise reproducible.
// The fused heads are built from the x-tile and row-walk helpers and the one per-pixel core (softmax_terms) of upsample_common.h;
// the inference tails live in upsample_infer.hip.
#include "upsample_common.h"

namespace {

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
    // thread t adds pairs t, t + 256, ... in ascending order (the order every CE head's loss bits rest on); the loads of 16 pairs are issued
    // together before their ordered adds, so one workgroup does not pay a memory round trip per pair (24 608 pairs at B = 8, 769 x 769)
    float s = 0.f, c = 0.f;
    const float2* pairs = reinterpret_cast<const float2*>(partial);
    int i = threadIdx.x;
    for (; i + 15 * 256 < n; i += 16 * 256) {
        float2 v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = pairs[i + j * 256];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            s += v[j].x;
            c += v[j].y;
        }
    }
    for (; i < n; i += 256) {
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
// pass 1 (an x-tile kernel): one workgroup per (b, y, tile of low-res columns).  Threads compute, ONCE per high-res pixel, the interpolated logits, the loss
// term and d = softmax - onehot into LDS; then (j,k) items gather the pixels of their column support in ascending x.
// MODE == UPCE_WEIGHTED (mi_upsample_ce_w): torch's CrossEntropyLoss(weight=, label_smoothing=s).  Per valid pixel, with lp_c = (z_c - max) - log(sum exp):
//   loss term = (1-s) w_y (-lp_y) + s/K sum_c w_c (-lp_c),  d_k = (1-s) w_y (p_k - [k==y]) + s/K (p_k Wsum - w_k),  "count" = w_y  (so that the
// finalize divides by S = sum_valid w_y and pass 2 by loss_out[1] as ever).  wce.cw (NULL: all 1) is read from device memory by every workgroup into
// LDS - K floats, a label-indexed ds_read per pixel instead of a global load - with Wsum behind them, added in class order.
// MODE == UPCE_PLAIN compiles none of it: wce is an unused kernel argument.
// MODE == UPCE_FOCAL (mi_upsample_ce_focal, gamma > 0): FL = -w_y (1 - p_y)^gamma log p_y.  Per valid pixel, with q = p_y, u = 1 - q, nll = -log q:
//   loss term = w_y u^gamma nll,  d_k = w_y m (p_k - [k==y]) with m = u^gamma (1 + gamma q nll / u),  "count" = w_y.
// u is the sum of the OTHER classes' v_k (class order) over the sum of all - not 1 - q, which has no relative precision left on a confident pixel - and
// nll is -log1p(-u) where u < 1/2 (log(sum) - picked rounds the sum to 1 + 6e-8 there).  m never forms u^(gamma-1) (infinite at u = 0 for gamma < 1):
// nll / u tends to 1 as u tends to 0 and is taken as 1 there, so u == 0 gives m = 0 and d = 0 exactly.  d_y is -u itself.  The LDS extras are the K
// class weights alone (no Wsum); wce.keep carries gamma.
enum { UPCE_PLAIN = 0, UPCE_WEIGHTED = 1, UPCE_FOCAL = 2 };
struct WceArgs {
    const float* cw;      // [K] class weights on the device, or NULL
    float keep;           // 1 - s          (UPCE_FOCAL: gamma)
    float smooth;         // s / K
};

struct WeightedSum {      // s += w_c (z_c - max), before the exponential for the same reason as `picked`
    const float* w;
    float& s;
    __device__ __forceinline__ void operator()(int k, float zk) const { s += w[k] * zk; }
};

__host__ __device__ inline TileLds upce_lds(int npx_max, int K, int mode) {      // UPCE_WEIGHTED: [K] class weights, then Wsum; UPCE_FOCAL: the weights
    return TileLds(npx_max, K, true, mode == UPCE_WEIGHTED ? K + 1 : mode == UPCE_FOCAL ? K : 0);
}

// u^gamma and m = u^gamma (1 + gamma q nll / u) of the focal loss for gamma > 0, 0 <= u <= 1; both 0 at u == 0.
__device__ __forceinline__ void focal_factors(float gamma, float u, float q, float nll, float& ug, float& m) {
    ug = u > 0.f ? exp2f(gamma * log2f(u)) : 0.f;
    const float ratio = u > 1e-30f ? nll / u : 1.f;
    m = ug * (1.f + gamma * (q * ratio));
}
__host__ __device__ inline TileLds grad_lds(int npx_max, int K) {      // the x-tile kernels that only write a gradient
    return TileLds(npx_max, K, false, 0);
}

template <int KT, int MODE = UPCE_PLAIN>
__global__ __launch_bounds__(256) void upce_pass1_kernel(const float* __restrict__ low, const int64_t* __restrict__ labels,
                                                         float* __restrict__ partial, float* __restrict__ tmp, int B, int Krt, Axis ay,
                                                         Axis ax, int ignore_index, int npx_max, unsigned* __restrict__ bad, int jt_cols, WceArgs wce) {
    const int K = KT > 0 ? KT : Krt;
    constexpr int KR = kreg<KT>;
    const XTile t = xtile_begin(upce_lds(npx_max, K, MODE), low, K, ay, ax, npx_max, jt_cols);
    float* wsh = t.extra;
    if constexpr (MODE == UPCE_FOCAL) {
        if (threadIdx.x < K) wsh[threadIdx.x] = wce.cw ? wce.cw[threadIdx.x] : 1.f;
    }
    if constexpr (MODE == UPCE_WEIGHTED) {
        if (threadIdx.x < K) wsh[threadIdx.x] = wce.cw ? wce.cw[threadIdx.x] : 1.f;
        __syncthreads();
        if (threadIdx.x == 0) {
            float s = 0.f;
            for (int k = 0; k < K; ++k) s += wsh[k];
            wsh[K] = s;
        }
    }
    __syncthreads();
    float loss = 0.f, cnt = 0.f;
    for (int px = threadIdx.x; px < t.npx; px += 256) {
        const XPixel q = xtile_pixel(t, ax, K, px);
        const long lab = labels[q.pix];
        float* d = q.d;
        if (q.own) count_bad_label(lab, K, ignore_index, bad);       // once per pixel: by the tile that owns it
        if (lab == ignore_index || lab < 0 || lab >= K) {
            for (int k = 0; k < K; ++k) d[k] = 0.f;
            continue;
        }
        float v[KR];
        float picked, wz = 0.f;
        float se;
        if constexpr (MODE == UPCE_WEIGHTED)
            se = softmax_terms<true>(q.c0, q.c1, q.lx, K, v, KR, lab, &picked, WeightedSum{wsh, wz});
        else
            se = softmax_terms<true>(q.c0, q.c1, q.lx, K, v, KR, lab, &picked);
        const float rse = 1.f / se;
        if constexpr (MODE == UPCE_FOCAL) {
            float other = 0.f, ey = 0.f;
#pragma unroll
            for (int k = 0; k < KR; ++k) {
                if (k < K) {
                    if (k == lab)
                        ey = v[k];
                    else
                        other += v[k];
                }
            }
            const float u = fminf(other * rse, 1.f), qy = ey * rse;
            const float nll = u < 0.5f ? -log1pf(-u) : __logf(se) - picked;
            float ug, m;
            focal_factors(wce.keep, u, qy, nll, ug, m);
            const float wy = wsh[lab], hard = wy * m;
#pragma unroll
            for (int k = 0; k < KR; ++k) {
                if (k < K) d[k] = hard * (k == lab ? -u : v[k] * rse);
            }
            if (q.own) {
                loss += (wy * ug) * nll;
                cnt += wy;
            }
            continue;
        }
        if constexpr (MODE == UPCE_WEIGHTED) {
            const float wy = wsh[lab], wsum = wsh[K];
            const float hard = wce.keep * wy;
#pragma unroll
            for (int k = 0; k < KR; ++k) {
                if (k < K) {
                    const float g = v[k] * rse - (k == lab ? 1.f : 0.f);
                    d[k] = hard * g + wce.smooth * ((v[k] * rse) * wsum - wsh[k]);
                }
            }
            if (q.own) {
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
        if (q.own) {
            loss += __logf(se) - picked;          // = logsumexp(x) - x[label], like ATen's log_softmax + nll_loss
            cnt += 1.f;
        }
    }
    __syncthreads();
    if (tmp) xtile_gather(t, tmp, K, ax.n_in);
    block_sum2(loss, cnt, t.red);
    if (threadIdx.x == 0) {
        const long pidx = t.row * gridDim.x + blockIdx.x;
        partial[2 * pidx] = loss;
        partial[2 * pidx + 1] = cnt;
    }
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

// partial: [workgroup][3K + 1] 32-bit words - T_c (unsigned), the bad-label count (unsigned), I_c (float), P2_c (float).
template <int KT>
__global__ __launch_bounds__(256) void gdl_reduce_kernel(const float* __restrict__ low, const int64_t* __restrict__ labels, unsigned* __restrict__ partial,
                                                         int Krt, Axis ay, Axis ax, int ignore_index, int rows, int ncol_max) {
    const int K = KT > 0 ? KT : Krt;
    constexpr int KR = kreg<KT>;
    extern __shared__ __attribute__((aligned(16))) float sh[];
    float* vrow = sh;                                                          // [ncol_max][K] source row already interpolated along y
    unsigned* red = reinterpret_cast<unsigned*>(sh + (long)ncol_max * K);      // [4][3K + 1]
    const int NC = 3 * K + 1, tid = threadIdx.x;
    const RowWalk r = rowwalk_begin(ay, ax, rows, ncol_max);
    float p2[KR], it[KR];
    unsigned tc[KR], bad = 0u;
#pragma unroll
    for (int k = 0; k < KR; ++k) {
        p2[k] = 0.f;
        it[k] = 0.f;
        tc[k] = 0u;
    }
    for (int y = r.ya; y < r.yb; ++y) {
        rowwalk_stage(r, low, vrow, K, ay, ax.n_in, y);
        if (r.live) {
            const long lab = labels[r.pix(ay, ax, y)];
            if (lab != ignore_index && lab >= 0 && lab < K) {
                float v[KR];
                const float rse = 1.f / softmax_terms(vrow + r.c0 * K, vrow + r.c1 * K, r.lx, K, v, KR);
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
        const long wg = ((long)r.b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        unsigned s;
        if (tid <= K)
            s = red[tid] + red[NC + tid] + red[2 * NC + tid] + red[3 * NC + tid];
        else
            s = __float_as_uint(((__uint_as_float(red[tid]) + __uint_as_float(red[NC + tid])) + __uint_as_float(red[2 * NC + tid])) +
                                __uint_as_float(red[3 * NC + tid]));
        partial[wg * NC + tid] = s;
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

// An x-tile kernel with d = d loss / d z of the Dice loss from the coefficients the finalize left in `coef` ([K] a_c, [K] b_c).
template <int KT>
__global__ __launch_bounds__(256) void gdl_grad_kernel(const float* __restrict__ low, const int64_t* __restrict__ labels, const float* __restrict__ coef,
                                                       float* __restrict__ tmp, int Krt, Axis ay, Axis ax, int ignore_index, int npx_max, int jt_cols) {
    const int K = KT > 0 ? KT : Krt;
    constexpr int KR = kreg<KT>;
    const XTile t = xtile_begin(grad_lds(npx_max, K), low, K, ay, ax, npx_max, jt_cols);
    __syncthreads();
    for (int px = threadIdx.x; px < t.npx; px += 256) {
        const XPixel q = xtile_pixel(t, ax, K, px);
        const long lab = labels[q.pix];
        float* d = q.d;
        if (lab == ignore_index || lab < 0 || lab >= K) {
            for (int k = 0; k < K; ++k) d[k] = 0.f;
            continue;
        }
        float v[KR];
        const float rse = 1.f / softmax_terms(q.c0, q.c1, q.lx, K, v, KR);
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
    xtile_gather(t, tmp, K, ax.n_in);
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
// SDF (mi_upsample_tversky_bce_sdf) is a mode of the three kernels: the boundary loss of Kervadec et al. on the signed distance map phi [B][H][W] of the
// label (mi_signed_distance), boundary = 1/N sum p phi, loss += w_bd boundary, d loss / d z += w_bd / N phi q.  One more 4-byte load per pixel in the
// reduction and the gradient pass, one more partial per workgroup (its own array: the four others stay one float4), one more coefficient.  With SDF
// false every addition is compiled out: the instantiations mi_upsample_tversky_bce launches are the kernels they were.
constexpr int TVB_NC = 4;          // TP, FN, FP, the bce sum

// p = sigmoid(z), np = 1 - p, e = exp(-|z|)
__device__ __forceinline__ void sigmoid_pair(float z, float& p, float& np, float& e) {
    e = __expf(-fabsf(z));
    const float r = 1.f / (1.f + e), er = e * r;
    p = z >= 0.f ? r : er;
    np = z >= 0.f ? er : r;
}

// A row-walk kernel with one channel.  partial: [workgroup][4] floats; SDF: partial_s [workgroup] floats, the sums of p phi.
template <bool SDF>
__global__ __launch_bounds__(256) void tvb_reduce_kernel(const float* __restrict__ low, const float* __restrict__ mask, float* __restrict__ partial, Axis ay,
                                                         Axis ax, int rows, const float* __restrict__ phi, float* __restrict__ partial_s) {
    __shared__ float vrow[GDL_XT + 2];          // source row already interpolated along y
    __shared__ float red[4][TVB_NC + (SDF ? 1 : 0)];
    const int tid = threadIdx.x;
    const RowWalk r = rowwalk_begin(ay, ax, rows, GDL_XT + 2);
    float tp = 0.f, fn = 0.f, fp = 0.f, bce = 0.f, sb = 0.f;
    for (int y = r.ya; y < r.yb; ++y) {
        rowwalk_stage(r, low, vrow, 1, ay, ax.n_in, y);
        if (r.live) {
            const float t = mask[r.pix(ay, ax, y)];
            const float z = (1.f - r.lx) * vrow[r.c0] + r.lx * vrow[r.c1];
            float p, np, e;
            sigmoid_pair(z, p, np, e);
            tp += p * t;
            fn += t * np;
            fp += p * (1.f - t);
            bce += (fmaxf(z, 0.f) - z * t) + log1pf(e);
            if constexpr (SDF) sb += p * phi[r.pix(ay, ax, y)];
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
    if constexpr (SDF) {
        sb = wave_sum(sb);
        if (lane == 0) red[wv][TVB_NC] = sb;
    }
    __syncthreads();
    if (tid < TVB_NC) {
        const long wg = ((long)r.b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        partial[wg * TVB_NC + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    }
    if constexpr (SDF) {
        if (tid == TVB_NC) {
            const long wg = ((long)r.b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
            partial_s[wg] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
        }
    }
}

// One workgroup: the partial rows added in fp64 in a fixed order (thread t takes rows t, t + 256, ...; butterfly per wave; the four waves in order), then
// loss_out = loss, tversky, bce, 0; coef = w_t c0, w_t c1, w_b / N; sums (nullable) = TP, FN, FP.
// SDF: loss_out[3] = boundary = S / N with S = sum p phi (0 when w_bd is 0), loss += w_bd boundary, coef[3] = w_bd / N, sums[3] = S.
template <bool SDF>
__global__ __launch_bounds__(256) void tvb_finalize_kernel(const float* __restrict__ partial, int n, double npix, float alpha, float eps, float w_t, float w_b,
                                                           float* __restrict__ loss_out, float* __restrict__ coef, float* __restrict__ sums,
                                                           const float* __restrict__ partial_s, float w_bd) {
    constexpr int NC = TVB_NC + (SDF ? 1 : 0);
    __shared__ double red[4][NC];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    double s[NC] = {};
    for (int i = tid; i < n; i += 256) {
        const float4 v = reinterpret_cast<const float4*>(partial)[i];
        s[0] += (double)v.x;
        s[1] += (double)v.y;
        s[2] += (double)v.z;
        s[3] += (double)v.w;
        if constexpr (SDF) s[TVB_NC] += (double)partial_s[i];
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        s[c] = wave_sum(s[c]);
        if (lane == 0) red[wv][c] = s[c];
    }
    __syncthreads();
    if (tid == 0) {
        double tot[NC];
        for (int c = 0; c < NC; ++c) tot[c] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
        const double a = (double)alpha, e = (double)eps, tpe = tot[0] + e;
        const double D = tot[0] + a * tot[1] + (1.0 - a) * tot[2] + e;          // >= eps > 0
        const double tversky = 1.0 - tpe / D, bce = tot[3] / npix;
        if constexpr (SDF) {
            const double boundary = w_bd > 0.f ? tot[TVB_NC] / npix : 0.0;          // w_bd == 0: the term is off, reported as the plain entry reports it
            loss_out[0] = (float)(((double)w_t * tversky + (double)w_b * bce) + (double)w_bd * boundary);
            loss_out[3] = (float)boundary;
            coef[3] = (float)((double)w_bd / npix);
            if (sums) sums[3] = (float)tot[TVB_NC];
        } else {
            loss_out[0] = (float)((double)w_t * tversky + (double)w_b * bce);
            loss_out[3] = 0.f;
        }
        loss_out[1] = (float)tversky;
        loss_out[2] = (float)bce;
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

// An x-tile kernel with one channel: d = d loss / d z from the three (SDF: four) coefficients the finalize left in `coef`; every pixel counts.
template <bool SDF>
__global__ __launch_bounds__(256) void tvb_grad_kernel(const float* __restrict__ low, const float* __restrict__ mask, const float* __restrict__ coef,
                                                       float* __restrict__ tmp, Axis ay, Axis ax, int npx_max, int jt_cols, const float* __restrict__ phi) {
    const XTile t = xtile_begin(grad_lds(npx_max, 1), low, 1, ay, ax, npx_max, jt_cols);
    __syncthreads();
    const float c0 = coef[0], c1 = coef[1], cb = coef[2];
    const float cd = SDF ? coef[3] : 0.f;
    for (int px = threadIdx.x; px < t.npx; px += 256) {
        const XPixel q = xtile_pixel(t, ax, 1, px);
        const float y = mask[q.pix];
        const float z = (1.f - q.lx) * q.c0[0] + q.lx * q.c1[0];
        float p, np, e;
        sigmoid_pair(z, p, np, e);
        if constexpr (SDF)
            q.d[0] = ((p * np) * (c1 - c0 * y) + cb * (p - y)) + (cd * phi[q.pix]) * (p * np);
        else
            q.d[0] = (p * np) * (c1 - c0 * y) + cb * (p - y);
    }
    __syncthreads();
    xtile_gather(t, tmp, 1, ax.n_in);
}

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
    constexpr int KR = kreg<KT>;
    extern __shared__ __attribute__((aligned(16))) float sh[];
    float* vrow = sh;                                                          // [ncol_max][K] source row already interpolated along y
    unsigned* lh = reinterpret_cast<unsigned*>(sh + (long)ncol_max * K);       // [OHEM_BINS]
    const int tid = threadIdx.x;
    for (int e = tid; e < OHEM_BINS; e += 256) lh[e] = 0u;
    const RowWalk r = rowwalk_begin(ay, ax, rows, ncol_max);
    unsigned nvalid = 0u, bad = 0u;
    for (int y = r.ya; y < r.yb; ++y) {
        rowwalk_stage(r, low, vrow, K, ay, ax.n_in, y);
        if (r.live) {
            const long pix = r.pix(ay, ax, y);
            const long lab = labels[pix];
            float q = OHEM_SENTINEL, nll = 0.f;
            if (lab != ignore_index && lab >= 0 && lab < K) {
                float v[KR];
                float picked, ey = 0.f;      // the loss term from picked = z_y - max before the exponential, as upce_pass1_kernel: finite when q underflows
                const float se = softmax_terms<true>(vrow + r.c0 * K, vrow + r.c1 * K, r.lx, K, v, KR, lab, &picked);
#pragma unroll
                for (int k = 0; k < KR; ++k) {
                    if (k < K && k == lab) ey = v[k];
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

// An x-tile kernel with d = kept (softmax - onehot); kept is read from the stored q (the sentinel of a pixel that is not valid lies above any t),
// and a pixel that is not kept costs neither a label read nor a softmax.
template <int KT>
__global__ __launch_bounds__(256) void ohem_grad_kernel(const float* __restrict__ low, const int64_t* __restrict__ labels, const float* __restrict__ q,
                                                        const unsigned* __restrict__ state, float* __restrict__ tmp, int Krt, Axis ay, Axis ax, int npx_max,
                                                        int jt_cols) {
    const int K = KT > 0 ? KT : Krt;
    constexpr int KR = kreg<KT>;
    const XTile t = xtile_begin(grad_lds(npx_max, K), low, K, ay, ax, npx_max, jt_cols);
    __syncthreads();
    const float thr = __uint_as_float(state[OHEM_T]);
    for (int px = threadIdx.x; px < t.npx; px += 256) {
        const XPixel p = xtile_pixel(t, ax, K, px);
        float* d = p.d;
        if (!(q[p.pix] <= thr)) {
            for (int k = 0; k < K; ++k) d[k] = 0.f;
            continue;
        }
        const long lab = labels[p.pix];
        float v[KR];
        const float rse = 1.f / softmax_terms(p.c0, p.c1, p.lx, K, v, KR);
#pragma unroll
        for (int k = 0; k < KR; ++k) {
            if (k < K) d[k] = v[k] * rse - (k == lab ? 1.f : 0.f);
        }
    }
    __syncthreads();
    xtile_gather(t, tmp, K, ax.n_in);
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

namespace {
// The fused CE head behind mi_upsample_ce_ex and mi_upsample_ce_w (which have checked their arguments).  Without weights and smoothing pass 1 is the
// PLAIN instantiation whichever entry was called: the compiler contracts the two instantiations differently (the plain <19> interpolates with two
// rounded products, the weighted one with an fma), so only the same code object makes "the defaults of mi_upsample_ce_w give mi_upsample_ce_ex's bits"
// hold whatever a later compiler does.  The weights travel as a device pointer, so a captured graph sees later values.
// zero_stays: the pass 2 that keeps exact zeros (wce_pass2_kernel).  focal_gamma > 0 (mi_upsample_ce_focal, without smoothing): the FOCAL instantiation;
// 0 is everything above, untouched.
int launch_upce(const char* who, const float* low, const int64_t* labels, const float* class_weights, float* loss_out, float* dlow, int B, int h, int w, int K,
                int H, int W, int ignore_index, float label_smoothing, float grad_scale, int align_corners, bool zero_stays, void* workspace,
                size_t workspace_bytes, hipStream_t st, float focal_gamma = 0.f) {
    if (workspace_bytes < mi_upsample_ce_workspace(B, h, w, K, H, W)) return mi_set_error(MI_ENOMEM, "%s: workspace too small", who);
    const HeadPlan p = head_plan(h, w, H, W, align_corners);
    float* partial = (float*)workspace;
    float* tmp = dlow ? (float*)((char*)workspace + up256((size_t)B * H * p.tiles * 2 * sizeof(float))) : nullptr;
    const bool focal = focal_gamma > 0.f, plain = !focal && !class_weights && label_smoothing == 0.f;
    const size_t lds = upce_lds(p.npx_max, K, focal ? UPCE_FOCAL : plain ? UPCE_PLAIN : UPCE_WEIGHTED).bytes();
    MI_REQUIRE(lds <= MI_LDS_MAX, "%s: upsample factor too large for one LDS tile (%zu B)", who, lds);
    const WceArgs wce{class_weights, focal ? focal_gamma : 1.f - label_smoothing, label_smoothing / (float)K};
    unsigned* bad = reinterpret_cast<unsigned*>(loss_out + 3);
    if (hipMemsetAsync(bad, 0, sizeof(unsigned), st) != hipSuccess) return mi_set_error(MI_EHIP, "%s: memset", who);
    with_kt(K, [&](auto kt) {
        constexpr int KT = decltype(kt)::value;
        if (focal)
            launch_xtile<upce_pass1_kernel<KT, UPCE_FOCAL>>(p, H, B, lds, st, low, labels, partial, tmp, B, K, p.ay, p.ax, ignore_index, p.npx_max, bad,
                                                            p.jt_cols, wce);
        else if (plain)
            launch_xtile<upce_pass1_kernel<KT, UPCE_PLAIN>>(p, H, B, lds, st, low, labels, partial, tmp, B, K, p.ay, p.ax, ignore_index, p.npx_max, bad,
                                                            p.jt_cols, wce);
        else
            launch_xtile<upce_pass1_kernel<KT, UPCE_WEIGHTED>>(p, H, B, lds, st, low, labels, partial, tmp, B, K, p.ay, p.ax, ignore_index, p.npx_max, bad,
                                                               p.jt_cols, wce);
    });
    if (int rc = launch_failed(who, "pass1")) return rc;
    hipLaunchKernelGGL(ce_finalize_kernel, dim3(1), dim3(256), 0, st, (const float*)partial, B * H * p.tiles, loss_out);
    if (int rc = launch_failed(who, "finalize")) return rc;
    if (dlow) {
        auto* pass2 = zero_stays ? wce_pass2_kernel : upce_pass2_kernel;
        hipLaunchKernelGGL(pass2, dim3(nblk((long)B * h * w * K, 256)), dim3(256), 0, st, (const float*)tmp,
                           (const float*)loss_out, dlow, B, K, p.ay, w, grad_scale);
        if (int rc = launch_failed(who, "pass2")) return rc;
    }
    return MI_OK;
}
}  // namespace

extern "C" int mi_upsample_ce_ex(const float* low, const int64_t* labels, float* loss_out, float* dlow, int B, int h, int w, int K, int H, int W,
                                 int ignore_index, float grad_scale, int align_corners, void* workspace, size_t workspace_bytes, void* stream) {
    MI_REQUIRE(low && labels && loss_out && workspace, "mi_upsample_ce: null operand");
    if (int rc = head_check("mi_upsample_ce", B, h, w, K, H, W)) return rc;
    return launch_upce("mi_upsample_ce", low, labels, nullptr, loss_out, dlow, B, h, w, K, H, W, ignore_index, 0.f, grad_scale, align_corners, false,
                       workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int mi_upsample_ce(const float* low, const int64_t* labels, float* loss_out, float* dlow, int B, int h, int w, int K, int H, int W,
                              int ignore_index, float grad_scale, void* workspace, size_t workspace_bytes, void* stream) {
    return mi_upsample_ce_ex(low, labels, loss_out, dlow, B, h, w, K, H, W, ignore_index, grad_scale, 1, workspace, workspace_bytes, stream);
}

// CrossEntropyLoss(weight=, ignore_index=, label_smoothing=) on the upsampled logits.
extern "C" int mi_upsample_ce_w(const float* low, const int64_t* labels, const float* class_weights, float* loss_out, float* dlow, int B, int h, int w,
                                int K, int H, int W, int ignore_index, float label_smoothing, float grad_scale, int align_corners, void* workspace,
                                size_t workspace_bytes, void* stream) {
    MI_REQUIRE(low && labels && loss_out && workspace, "mi_upsample_ce_w: null operand");
    if (int rc = head_check("mi_upsample_ce_w", B, h, w, K, H, W)) return rc;
    MI_REQUIRE(std::isfinite(label_smoothing), "mi_upsample_ce_w: label_smoothing is not finite");
    MI_REQUIRE(label_smoothing >= 0.f && label_smoothing <= 1.f, "mi_upsample_ce_w: label_smoothing outside [0, 1]");
    MI_REQUIRE(std::isfinite(grad_scale), "mi_upsample_ce_w: grad_scale is not finite");
    return launch_upce("mi_upsample_ce_w", low, labels, class_weights, loss_out, dlow, B, h, w, K, H, W, ignore_index, label_smoothing, grad_scale,
                       align_corners, true, workspace, workspace_bytes, (hipStream_t)stream);
}

// Focal loss FL = -w_y (1 - p_y)^gamma log p_y on the upsampled logits, normalised by the weight sum of the valid pixels.  gamma == 0 is
// mi_upsample_ce_w at label_smoothing 0: the same launches, the same bits.
extern "C" int mi_upsample_ce_focal(const float* low, const int64_t* labels, const float* class_weights, float* loss_out, float* dlow, int B, int h, int w,
                                    int K, int H, int W, int ignore_index, float gamma, float grad_scale, int align_corners, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    MI_REQUIRE(low && labels && loss_out && workspace, "mi_upsample_ce_focal: null operand");
    if (int rc = head_check("mi_upsample_ce_focal", B, h, w, K, H, W)) return rc;
    MI_REQUIRE(std::isfinite(gamma), "mi_upsample_ce_focal: gamma is not finite");
    MI_REQUIRE(gamma >= 0.f && gamma <= 8.f, "mi_upsample_ce_focal: gamma outside [0, 8]");
    MI_REQUIRE(std::isfinite(grad_scale), "mi_upsample_ce_focal: grad_scale is not finite");
    return launch_upce("mi_upsample_ce_focal", low, labels, class_weights, loss_out, dlow, B, h, w, K, H, W, ignore_index, 0.f, grad_scale, align_corners,
                       true, workspace, workspace_bytes, (hipStream_t)stream, gamma);
}

extern "C" size_t mi_upsample_gdl_workspace(int B, int h, int w, int K, int H, int W) {
    if (B <= 0 || h <= 0 || w <= 0 || K <= 0 || H <= 0 || W <= 0) return 0;
    const GdlPlan p = gdl_plan(B, H, W);
    return up256(p.nwg * (3 * (size_t)K + 1) * sizeof(unsigned)) + up256(2 * (size_t)K * sizeof(float)) + (size_t)B * H * w * K * sizeof(float);
}

extern "C" int mi_upsample_gdl(const float* low, const int64_t* labels, float* loss_out, float* dlow, float* sums, int B, int h, int w, int K, int H,
                               int W, int ignore_index, int weight_type, float eps, float grad_scale, int align_corners, void* workspace,
                               size_t workspace_bytes, void* stream) {
    MI_REQUIRE(low && labels && loss_out && workspace, "mi_upsample_gdl: null operand");
    if (int rc = head_check("mi_upsample_gdl", B, h, w, K, H, W)) return rc;
    MI_REQUIRE(weight_type >= MI_GDL_SQUARE && weight_type <= MI_GDL_SQRT, "mi_upsample_gdl: weight_type is MI_GDL_SQUARE, MI_GDL_IDENTITY or MI_GDL_SQRT");
    MI_REQUIRE(eps > 0.f, "mi_upsample_gdl: eps must be positive");
    if (workspace_bytes < mi_upsample_gdl_workspace(B, h, w, K, H, W)) return mi_set_error(MI_ENOMEM, "mi_upsample_gdl: workspace too small");
    const HeadPlan p = head_plan(h, w, H, W, align_corners);
    const GdlPlan pl = gdl_plan(B, H, W);
    hipStream_t st = (hipStream_t)stream;
    unsigned* partial = (unsigned*)workspace;
    float* coef = (float*)((char*)workspace + up256(pl.nwg * (3 * (size_t)K + 1) * sizeof(unsigned)));
    float* tmp = (float*)((char*)coef + up256(2 * (size_t)K * sizeof(float)));
    const int ncol_max = w < GDL_XT + 2 ? w : GDL_XT + 2;
    const size_t lds1 = ((size_t)ncol_max * K + 4 * (3 * (size_t)K + 1)) * 4;          // <= 34 KB
    const size_t lds3 = grad_lds(p.npx_max, K).bytes();
    MI_REQUIRE(!dlow || lds3 <= MI_LDS_MAX, "mi_upsample_gdl: upsample factor too large for one LDS tile (%zu B)", lds3);
    with_kt(K, [&](auto kt) {
        hipLaunchKernelGGL(gdl_reduce_kernel<decltype(kt)::value>, dim3(pl.tiles_x, pl.row_groups, B), dim3(256), lds1, st, low, labels, partial, K, p.ay, p.ax,
                           ignore_index, pl.rows, ncol_max);
    });
    MI_CHECK_LAUNCH("mi_upsample_gdl reduce");
    hipLaunchKernelGGL(gdl_finalize_kernel, dim3(1), dim3(64 * GDL_FIN_WAVES), 0, st, (const unsigned*)partial, (int)pl.nwg, K, weight_type, eps, loss_out, coef,
                       sums);
    MI_CHECK_LAUNCH("mi_upsample_gdl finalize");
    if (dlow) {
        with_kt(K, [&](auto kt) {
            launch_xtile<gdl_grad_kernel<decltype(kt)::value>>(p, H, B, lds3, st, low, labels, (const float*)coef, tmp, K, p.ay, p.ax, ignore_index, p.npx_max,
                                                               p.jt_cols);
        });
        MI_CHECK_LAUNCH("mi_upsample_gdl gradient");
        hipLaunchKernelGGL(upce_pass2_kernel, dim3(nblk((long)B * h * w * K, 256)), dim3(256), 0, st, (const float*)tmp, (const float*)nullptr, dlow, B, K, p.ay,
                           w, grad_scale);
        MI_CHECK_LAUNCH("mi_upsample_gdl gradient rows");
    }
    return MI_OK;
}

// The workspace of both Tversky + BCE entries: the float4 partials, (sdf) the partial sums of p phi, the coefficients, the x pass's output.
struct TvbWs {
    size_t partial_s, coef, tmp, total;
};
static TvbWs tvb_layout(int B, int w, int H, int W, bool sdf) {
    const GdlPlan p = gdl_plan(B, H, W);
    TvbWs l;
    l.partial_s = up256(p.nwg * TVB_NC * sizeof(float));
    l.coef = l.partial_s + (sdf ? up256(p.nwg * sizeof(float)) : 0);
    l.tmp = l.coef + up256((sdf ? 4 : 3) * sizeof(float));
    l.total = l.tmp + (size_t)B * H * w * sizeof(float);
    return l;
}

extern "C" size_t mi_upsample_tversky_bce_workspace(int B, int h, int w, int H, int W) {
    if (B <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return 0;
    return tvb_layout(B, w, H, W, false).total;
}

extern "C" size_t mi_upsample_tversky_bce_sdf_workspace(int B, int h, int w, int H, int W) {
    if (B <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return 0;
    return tvb_layout(B, w, H, W, true).total;
}

// Both entries: phi == nullptr is mi_upsample_tversky_bce (`who`), else the SDF instantiations.
template <bool SDF>
static int tvb_launch(const char* who, const float* low, const float* mask, const float* phi, float* loss_out, float* dlow, float* sums, int B, int h, int w,
                      int H, int W, float alpha, float eps, float w_tversky, float w_bce, float w_boundary, float grad_scale, int align_corners, void* workspace,
                      size_t workspace_bytes, void* stream) {
    if (int rc = head_check(who, B, h, w, 1, H, W, "")) return rc;
    MI_REQUIRE(alpha >= 0.f && alpha <= 1.f, "%s: alpha outside [0, 1]", who);          // (a NaN fails both comparisons)
    MI_REQUIRE(eps > 0.f, "%s: eps must be positive", who);
    const TvbWs l = tvb_layout(B, w, H, W, SDF);
    if (workspace_bytes < l.total) return mi_set_error(MI_ENOMEM, "%s: workspace too small", who);
    const HeadPlan p = head_plan(h, w, H, W, align_corners);
    const GdlPlan pl = gdl_plan(B, H, W);
    hipStream_t st = (hipStream_t)stream;
    float* partial = (float*)workspace;
    float* partial_s = (float*)((char*)workspace + l.partial_s);
    float* coef = (float*)((char*)workspace + l.coef);
    float* tmp = (float*)((char*)workspace + l.tmp);
    const size_t lds3 = grad_lds(p.npx_max, 1).bytes();          // within the 64 KB every kernel may use: launched without launch_xtile's opt-in
    MI_REQUIRE(!dlow || lds3 <= 64 * 1024, "%s: upsample factor too large for one LDS tile (%zu B)", who, lds3);
    hipLaunchKernelGGL(tvb_reduce_kernel<SDF>, dim3(pl.tiles_x, pl.row_groups, B), dim3(256), 0, st, low, mask, partial, p.ay, p.ax, pl.rows, phi, partial_s);
    MI_CHECK_LAUNCH("mi_upsample_tversky_bce reduce");
    hipLaunchKernelGGL(tvb_finalize_kernel<SDF>, dim3(1), dim3(256), 0, st, (const float*)partial, (int)pl.nwg, (double)B * H * W, alpha, eps, w_tversky, w_bce,
                       loss_out, coef, sums, (const float*)partial_s, w_boundary);
    MI_CHECK_LAUNCH("mi_upsample_tversky_bce finalize");
    if (dlow) {
        hipLaunchKernelGGL(tvb_grad_kernel<SDF>, dim3(p.tiles, H, B), dim3(256), lds3, st, low, mask, (const float*)coef, tmp, p.ay, p.ax, p.npx_max, p.jt_cols,
                           phi);
        MI_CHECK_LAUNCH("mi_upsample_tversky_bce gradient");
        hipLaunchKernelGGL(upce_pass2_kernel, dim3(nblk((long)B * h * w, 256)), dim3(256), 0, st, (const float*)tmp, (const float*)nullptr, dlow, B, 1, p.ay, w,
                           grad_scale);
        MI_CHECK_LAUNCH("mi_upsample_tversky_bce gradient rows");
    }
    return MI_OK;
}

extern "C" int mi_upsample_tversky_bce(const float* low, const float* mask, float* loss_out, float* dlow, float* sums, int B, int h, int w, int H, int W,
                                       float alpha, float eps, float w_tversky, float w_bce, float grad_scale, int align_corners, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    MI_REQUIRE(low && mask && loss_out && workspace, "mi_upsample_tversky_bce: null operand");
    return tvb_launch<false>("mi_upsample_tversky_bce", low, mask, nullptr, loss_out, dlow, sums, B, h, w, H, W, alpha, eps, w_tversky, w_bce, 0.f, grad_scale,
                             align_corners, workspace, workspace_bytes, stream);
}

extern "C" int mi_upsample_tversky_bce_sdf(const float* low, const float* mask, const float* phi, float* loss_out, float* dlow, float* sums, int B, int h, int w,
                                           int H, int W, float alpha, float eps, float w_tversky, float w_bce, float w_boundary, float grad_scale,
                                           int align_corners, void* workspace, size_t workspace_bytes, void* stream) {
    MI_REQUIRE(low && mask && phi && loss_out && workspace, "mi_upsample_tversky_bce_sdf: null operand");
    MI_REQUIRE(w_boundary >= 0.f && std::isfinite(w_boundary), "mi_upsample_tversky_bce_sdf: w_boundary must be finite and not negative");
    return tvb_launch<true>("mi_upsample_tversky_bce_sdf", low, mask, phi, loss_out, dlow, sums, B, h, w, H, W, alpha, eps, w_tversky, w_bce, w_boundary,
                            grad_scale, align_corners, workspace, workspace_bytes, stream);
}

extern "C" size_t mi_upsample_ce_ohem_workspace(int B, int h, int w, int K, int H, int W) {
    if (B <= 0 || h <= 0 || w <= 0 || K <= 0 || H <= 0 || W <= 0) return 0;
    return ohem_layout(B, w, K, H, W).total;
}

extern "C" int mi_upsample_ce_ohem(const float* low, const int64_t* labels, float* loss_out, float* dlow, float* prob, int B, int h, int w, int K, int H,
                                   int W, int ignore_index, float thresh, int64_t min_kept, float grad_scale, int align_corners, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    MI_REQUIRE(low && labels && loss_out && workspace, "mi_upsample_ce_ohem: null operand");
    if (int rc = head_check("mi_upsample_ce_ohem", B, h, w, K, H, W)) return rc;
    MI_REQUIRE((long)B * H * W < (1L << 24), "mi_upsample_ce_ohem: B H W must stay below 2^24 (n_kept is reported as a float)");
    MI_REQUIRE(thresh >= 0.f && thresh <= 1.f, "mi_upsample_ce_ohem: thresh outside [0, 1]");          // (a NaN fails both comparisons)
    MI_REQUIRE(min_kept >= 1, "mi_upsample_ce_ohem: min_kept must be at least 1");
    MI_REQUIRE(std::isfinite(grad_scale), "mi_upsample_ce_ohem: grad_scale is not finite");
    if (workspace_bytes < mi_upsample_ce_ohem_workspace(B, h, w, K, H, W)) return mi_set_error(MI_ENOMEM, "mi_upsample_ce_ohem: workspace too small");
    const HeadPlan p = head_plan(h, w, H, W, align_corners);
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
    const size_t lds3 = grad_lds(p.npx_max, K).bytes();
    MI_REQUIRE(!dlow || lds3 <= MI_LDS_MAX, "mi_upsample_ce_ohem: upsample factor too large for one LDS tile (%zu B)", lds3);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(hist, 0, (3 * OHEM_BINS + OHEM_STATE) * sizeof(unsigned), st) != hipSuccess) return mi_set_error(MI_EHIP, "mi_upsample_ce_ohem: memset");
    with_kt(K, [&](auto kt) {
        hipLaunchKernelGGL(ohem_prob_kernel<decltype(kt)::value>, dim3(pl.tiles_x, pl.row_groups, B), dim3(256), lds1, st, low, labels, q, nll, hist, state, K,
                           p.ay, p.ax, ignore_index, pl.rows, ncol_max);
    });
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
        with_kt(K, [&](auto kt) {
            launch_xtile<ohem_grad_kernel<decltype(kt)::value>>(p, H, B, lds3, st, low, labels, (const float*)q, (const unsigned*)state, tmp, K, p.ay, p.ax,
                                                                p.npx_max, p.jt_cols);
        });
        MI_CHECK_LAUNCH("mi_upsample_ce_ohem gradient");
        hipLaunchKernelGGL(wce_pass2_kernel, dim3(nblk((long)B * h * w * K, 256)), dim3(256), 0, st, (const float*)tmp, (const float*)loss_out, dlow, B, K, p.ay, w,
                           grad_scale);
        MI_CHECK_LAUNCH("mi_upsample_ce_ohem gradient rows");
    }
    if (prob && hipMemcpyAsync(prob, q, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
        return mi_set_error(MI_EHIP, "mi_upsample_ce_ohem: copy of q");
    return MI_OK;
}
