// Lovasz-Softmax (Berman, Triki, Blaschko, CVPR 2018; classes = 'present', over the whole batch) fused with the bilinear upsample, on a 1024-cell order
// instead of a sort.  With z = bilinear(low), p = softmax(z), valid = label is not ignore_index and lies in [0, K), for every class c:
//   e_i = 1 - p_i[c] where y_i == c (foreground), p_i[c] elsewhere (background);  cell_i = min(1023, floor(e_i * 1024))
//   F[b], N[b] = foreground / background pixels in cell b;  G = sum F;  a_b, n_b = foreground / background pixels in strictly higher cells
//   g_fg[b] = 1 / (G + n_b);  g_bg[b] = (G - a_b - F[b]) / ((G + n_b) (G + n_b + N[b]))
//   loss_c = sum_i e_i g[cell_i];  loss = mean of loss_c over the classes with G > 0
// That is the Lovasz gradient of the order "descending cell; inside a cell the foreground pixels first, then the background pixels with their Jaccard
// increments averaged": a valid subgradient (ties), so 0 <= exact - loss <= 1/1024 per class.  Nothing differentiates through the cells:
//   d loss / d z_k = p_k (s_k - sum_c s_c p_c),  s_c = -g_fg / C on the foreground, +g_bg / C on the background, C = number of present classes.
// Launches (nothing is read back, so the call can be captured):
//   memset of the count table and the three state words
//   lovasz_count_kernel     row-walk: the K errors of every valid pixel into a per-workgroup LDS table of packed 16-bit pairs (F low, N high), merged into
//                           the [K][1024][2] table with integer atomics.  The background count of cell 0 is never incremented (the scan forms it).
//   lovasz_scan_kernel      one workgroup per class: N[0] = n_valid - G - sum_{b>0} N[b], suffix sums, the coefficients in fp64 stored as fp32, C
//   lovasz_grad_kernel      x-tile: softmax again, K coefficient lookups, a per-tile loss partial and d gathered along x
//   lovasz_finalize_kernel  one workgroup: the partials in fp64 in a fixed order, loss_out
//   lovasz_pass2_kernel     pass2_body along y
// Every pass takes its e from lovasz_errors on a row staged with lerp_rounded: the cells of the gradient are the cells that were counted.
#include "upsample_common.h"

namespace {

constexpr int LOV_BINS = 1024;
enum { LOV_NVALID = 0, LOV_BAD = 1, LOV_PRESENT = 2, LOV_STATE = 8 };          // the words behind the count table
constexpr float LOV_SENTINEL = 2.f;
constexpr int LOV_MAX_ROWS = 255;          // rows per workgroup of the counting pass: 255 * 256 pixels fit a 16-bit counter
constexpr int LOV_PEEL = 2;                // in-wave aggregation rounds before the LDS add (lds_hist_add's idea, upsample_infer.hip)

// The probabilities of one pixel from its two staged columns into v[0 .. K), and the foreground error of class `lab` as (sum of the other classes'
// exponentials) / (sum of all): 1 - p has no relative precision left on a confident pixel.  e of class k is the return value for k == lab and v[k]
// elsewhere.  Contraction is off, so the two kernels that call this round alike.  (v and kr as in exp_terms.)
__device__ __forceinline__ float lovasz_errors(const float* c0, const float* c1, float lx, int K, int kr, int lab, float* v) {
#pragma clang fp contract(off)
    float mx = -3.0e38f;
#pragma unroll
    for (int k = 0; k < kr; ++k) {
        if (k < K) {
            v[k] = lerp_rounded(lx, c0[k], c1[k]);
            mx = fmaxf(mx, v[k]);
        }
    }
    float se = 0.f, other = 0.f;
#pragma unroll
    for (int k = 0; k < kr; ++k) {
        if (k < K) {
            v[k] = __expf(v[k] - mx);
            se += v[k];
            if (k != lab) other += v[k];
        }
    }
    const float rse = 1.f / se;
#pragma unroll
    for (int k = 0; k < kr; ++k) {
        if (k < K) v[k] = v[k] * rse;
    }
    return fminf(other * rse, 1.f);
}

__device__ __forceinline__ int lovasz_cell(float e) {          // a power-of-two scale and a truncation, both exact; the lower clamp only keeps a NaN in bounds
    return min(LOV_BINS - 1, max(0, (int)(e * (float)LOV_BINS)));
}

// One (pixel, class) into the workgroup's table (tab: [1024] packed pairs of the class) or, without a table, into the class's [1024][2] counters in
// memory.  An untrained net puts a wave's 64 errors of one class into a few neighbouring cells, which an LDS atomic serialises; so first LOV_PEEL rounds
// of in-wave aggregation: the lanes that hold the key of the first lane still waiting retire, and their leader carries their number.
__device__ __forceinline__ void lovasz_add(unsigned* tab, unsigned* __restrict__ hist, bool want, int cell, bool fg, int lane) {
    const unsigned key = (unsigned)cell * 2u + (fg ? 0u : 1u);
    unsigned add = want ? 1u : 0u;
    bool waiting = want;
#pragma unroll
    for (int r = 0; r < LOV_PEEL; ++r) {
        if (waiting) {
            const unsigned k0 = (unsigned)__builtin_amdgcn_readfirstlane((int)key);
            const bool same = key == k0;
            const unsigned long long m = __ballot(same);          // among the lanes still waiting
            if (same) {
                waiting = false;
                add = lane == __ffsll((long long)m) - 1 ? (unsigned)__popcll(m) : 0u;
            }
        }
    }
    if (add) {
        if (tab)
            atomicAdd(&tab[cell], fg ? add : add << 16);
        else
            atomicAdd(&hist[key], add);
    }
}

// A row-walk kernel.  LDS: vrow [ncol_max][K], then (with_table) K * 1024 packed counters.  err (nullable): [B][K][H][W].
template <int KT>
__global__ __launch_bounds__(256) void lovasz_count_kernel(const float* __restrict__ low, const int64_t* __restrict__ labels, unsigned* __restrict__ hist,
                                                           unsigned* __restrict__ state, float* __restrict__ err, int Krt, Axis ay, Axis ax, int ignore_index,
                                                           int rows, int ncol_max, int with_table) {
    const int K = KT > 0 ? KT : Krt;
    constexpr int KR = kreg<KT>;
    extern __shared__ __attribute__((aligned(16))) float sh[];
    float* vrow = sh;
    unsigned* tab = with_table ? reinterpret_cast<unsigned*>(sh + (long)ncol_max * K) : nullptr;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tab) {
        for (int e = tid; e < K * LOV_BINS; e += 256) tab[e] = 0u;          // (published by the barrier of the first rowwalk_stage)
    }
    const RowWalk r = rowwalk_begin(ay, ax, rows, ncol_max);
    const long plane = (long)ay.n_out * ax.n_out;
    unsigned nvalid = 0u, bad = 0u;
    for (int y = r.ya; y < r.yb; ++y) {
        rowwalk_stage<true>(r, low, vrow, K, ay, ax.n_in, y);
        if (r.live) {
            const long lab = labels[r.pix(ay, ax, y)];
            float* eo = err ? err + ((long)r.b * K * ay.n_out + y) * ax.n_out + r.x : nullptr;
            if (lab != ignore_index && lab >= 0 && lab < K) {
                float v[KR];
                const float efg = lovasz_errors(vrow + r.c0 * K, vrow + r.c1 * K, r.lx, K, KR, (int)lab, v);
                nvalid += 1u;
#pragma unroll
                for (int k = 0; k < KR; ++k) {
                    if (k < K) {
                        const bool fg = k == lab;
                        const float e = fg ? efg : v[k];
                        const int cell = lovasz_cell(e);
                        lovasz_add(tab ? tab + k * LOV_BINS : nullptr, hist + (long)k * LOV_BINS * 2, fg || cell > 0, cell, fg, lane);
                        if (eo) eo[k * plane] = e;
                    }
                }
            } else {
                if (lab != ignore_index) bad += 1u;
                if (eo) {
                    for (int k = 0; k < K; ++k) eo[k * plane] = LOV_SENTINEL;
                }
            }
        }
        __syncthreads();          // the next row overwrites vrow; after the last row: the table is complete
    }
    nvalid = wave_sum(nvalid);
    bad = wave_sum(bad);
    if (lane == 0) {
        if (nvalid) atomicAdd(&state[LOV_NVALID], nvalid);
        if (bad) atomicAdd(&state[LOV_BAD], bad);
    }
    if (tab) {
        for (int e = tid; e < K * LOV_BINS; e += 256) {
            const unsigned c = tab[e];
            if (c & 0xffffu) atomicAdd(&hist[2 * e], c & 0xffffu);
            if (c >> 16) atomicAdd(&hist[2 * e + 1], c >> 16);
        }
    }
}

// One workgroup per class; thread t owns cells 4t .. 4t + 3.  Completes hist with N[0], writes coef [K][1024][2] (g_fg, g_bg; zeros for a class that
// is not present) and counts the present classes.  Counts are integers, the coefficients are formed in fp64.
__global__ __launch_bounds__(256) void lovasz_scan_kernel(unsigned* __restrict__ hist_all, unsigned* __restrict__ state, float* __restrict__ coef_all) {
    __shared__ unsigned sf[256], sn[256];
    const int tid = threadIdx.x, c = blockIdx.x;
    unsigned* hist = hist_all + (long)c * LOV_BINS * 2;
    float* coef = coef_all + (long)c * LOV_BINS * 2;
    unsigned F[4], N[4], f = 0u, n = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        F[i] = hist[(tid * 4 + i) * 2];
        N[i] = hist[(tid * 4 + i) * 2 + 1];          // cell 0: still 0
        f += F[i];
        n += N[i];
    }
    sf[tid] = f;
    sn[tid] = n;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {          // inclusive scans of the 256 thread sums
        const unsigned a = tid >= d ? sf[tid - d] : 0u, b = tid >= d ? sn[tid - d] : 0u;
        __syncthreads();
        sf[tid] += a;
        sn[tid] += b;
        __syncthreads();
    }
    const unsigned G = sf[255], NS = sn[255];
    if (tid == 0) {
        N[0] = state[LOV_NVALID] - G - NS;
        hist[1] = N[0];
        if (G) atomicAdd(&state[LOV_PRESENT], 1u);
    }
    unsigned a = G - sf[tid], nh = NS - sn[tid];          // foreground / background pixels in the cells above this thread's four
#pragma unroll
    for (int i = 3; i >= 0; --i) {
        float gf = 0.f, gb = 0.f;
        if (G) {
            const double D = (double)G + (double)nh;
            gf = (float)(1.0 / D);
            gb = (float)(((double)G - (double)a - (double)F[i]) / (D * (D + (double)N[i])));
        }
        coef[(tid * 4 + i) * 2] = gf;
        coef[(tid * 4 + i) * 2 + 1] = gb;
        a += F[i];
        nh += N[i];
    }
}

__host__ __device__ inline TileLds lovasz_lds(int npx_max, int K) { return TileLds(npx_max, K, true, 0); }

// An x-tile kernel: partial[row * tiles + tile] = sum over the tile's own pixels of sum_c e g (not yet divided by C), and - with tmp - d loss / d z
// gathered along x.
template <int KT>
__global__ __launch_bounds__(256) void lovasz_grad_kernel(const float* __restrict__ low, const int64_t* __restrict__ labels, const float* __restrict__ coef,
                                                          const unsigned* __restrict__ state, float* __restrict__ partial, float* __restrict__ tmp, int Krt,
                                                          Axis ay, Axis ax, int ignore_index, int npx_max, int jt_cols) {
    const int K = KT > 0 ? KT : Krt;
    constexpr int KR = kreg<KT>;
    const XTile t = xtile_begin<true>(lovasz_lds(npx_max, K), low, K, ay, ax, npx_max, jt_cols);
    __syncthreads();
    const unsigned C = state[LOV_PRESENT];
    const float inv_c = C ? 1.f / (float)C : 0.f;
    float loss = 0.f, unused = 0.f;
    for (int px = threadIdx.x; px < t.npx; px += 256) {
        const XPixel q = xtile_pixel(t, ax, K, px);
        const long lab = labels[q.pix];
        float* d = q.d;
        if (lab == ignore_index || lab < 0 || lab >= K) {
            for (int k = 0; k < K; ++k) d[k] = 0.f;
            continue;
        }
        float v[KR];
        const float efg = lovasz_errors(q.c0, q.c1, q.lx, K, KR, (int)lab, v);
        float l = 0.f, sp = 0.f;          // sum_c e_c g_c;  sum_c s_c p_c
#pragma unroll
        for (int k = 0; k < KR; ++k) {
            if (k < K) {
                const bool fg = k == lab;
                const float e = fg ? efg : v[k];
                const float g = coef[((long)k * LOV_BINS + lovasz_cell(e)) * 2 + (fg ? 0 : 1)];
                l += e * g;
                const float sk = (fg ? -g : g) * inv_c;
                d[k] = sk;          // s_k waits in the pixel's slot: a second register array spills the generic instantiation
                sp += sk * v[k];
            }
        }
#pragma unroll
        for (int k = 0; k < KR; ++k) {
            if (k < K) d[k] = v[k] * (d[k] - sp);
        }
        if (q.own) loss += l;
    }
    __syncthreads();
    if (tmp) xtile_gather(t, tmp, K, ax.n_in);
    block_sum2(loss, unused, t.red);
    if (threadIdx.x == 0) partial[t.row * gridDim.x + blockIdx.x] = loss;
}

// One workgroup: thread t adds partials t, t + 256, ... in fp64, the wave by butterfly, the four waves in order.
// loss_out = loss, valid pixels, out-of-range labels, present classes.
__global__ __launch_bounds__(256) void lovasz_finalize_kernel(const float* __restrict__ partial, long n, const unsigned* __restrict__ state,
                                                              float* __restrict__ loss_out) {
    __shared__ double rs[4];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (long i = tid; i < n; i += 256) s += (double)partial[i];
    s = wave_sum(s);
    if ((tid & 63) == 0) rs[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        const double tot = ((rs[0] + rs[1]) + rs[2]) + rs[3];
        const unsigned C = state[LOV_PRESENT];
        loss_out[0] = (float)(tot / (double)C);          // 0 / 0 = nan when no pixel is valid, as the other heads
        loss_out[1] = (float)state[LOV_NVALID];
        loss_out[2] = (float)state[LOV_BAD];
        loss_out[3] = (float)C;
    }
}

__global__ void lovasz_pass2_kernel(const float* __restrict__ tmp, float* __restrict__ dlow, int B, int K, Axis ay, int w, float grad_scale) {
    pass2_body<false>(tmp, nullptr, dlow, B, K, ay, w, grad_scale);
}

// The row-walk grid of the counting pass: gdl_plan with the rows of a workgroup capped at LOV_MAX_ROWS.
inline GdlPlan lovasz_plan(int B, int H, int W) {
    GdlPlan p = gdl_plan(B, H, W);
    if (p.rows > LOV_MAX_ROWS) {
        p.rows = LOV_MAX_ROWS;
        p.row_groups = (H + p.rows - 1) / p.rows;
        p.nwg = (size_t)B * p.row_groups * p.tiles_x;
    }
    return p;
}

struct LovaszLayout {
    size_t hist, coef, partial, tmp, total;
};
inline LovaszLayout lovasz_layout(int B, int h, int w, int K, int H, int W) {
    LovaszLayout l;
    const HeadPlan p = head_plan(h, w, H, W, 1);          // (the tile count does not depend on the convention)
    l.hist = 0;
    l.coef = l.hist + up256(((size_t)K * LOV_BINS * 2 + LOV_STATE) * sizeof(unsigned));
    l.partial = l.coef + up256((size_t)K * LOV_BINS * 2 * sizeof(float));
    l.tmp = l.partial + up256((size_t)B * H * p.tiles * sizeof(float));
    l.total = l.tmp + (size_t)B * H * w * K * sizeof(float);
    return l;
}

}  // namespace

extern "C" size_t mi_upsample_lovasz_workspace(int B, int h, int w, int K, int H, int W) {
    if (B <= 0 || h <= 0 || w <= 0 || K <= 0 || H <= 0 || W <= 0) return 0;
    return lovasz_layout(B, h, w, K, H, W).total;
}

extern "C" int mi_upsample_lovasz(const float* low, const int64_t* labels, float* loss_out, float* dlow, uint32_t* hist_out, float* err, int B, int h, int w,
                                  int K, int H, int W, int ignore_index, int bins, float grad_scale, int align_corners, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    MI_REQUIRE(low && labels && loss_out && workspace, "mi_upsample_lovasz: null operand");
    if (int rc = head_check("mi_upsample_lovasz", B, h, w, K, H, W)) return rc;
    MI_REQUIRE(bins == LOV_BINS, "mi_upsample_lovasz: bins must be 1024");
    MI_REQUIRE((long)B * H * W < (1L << 31), "mi_upsample_lovasz: B H W must stay below 2^31 (32-bit counters)");
    MI_REQUIRE(std::isfinite(grad_scale), "mi_upsample_lovasz: grad_scale is not finite");
    if (workspace_bytes < mi_upsample_lovasz_workspace(B, h, w, K, H, W)) return mi_set_error(MI_ENOMEM, "mi_upsample_lovasz: workspace too small");
    const HeadPlan p = head_plan(h, w, H, W, align_corners);
    const GdlPlan pl = lovasz_plan(B, H, W);
    const LovaszLayout lay = lovasz_layout(B, h, w, K, H, W);
    char* ws = (char*)workspace;
    unsigned* hist = (unsigned*)(ws + lay.hist);
    unsigned* state = hist + (size_t)K * LOV_BINS * 2;
    float* coef = (float*)(ws + lay.coef);
    float* partial = (float*)(ws + lay.partial);
    float* tmp = dlow ? (float*)(ws + lay.tmp) : nullptr;
    const int ncol_max = w < GDL_XT + 2 ? w : GDL_XT + 2;
    const size_t lds_row = (size_t)ncol_max * K * 4, lds_tab = (size_t)K * LOV_BINS * 4;
    const int with_table = lds_row + lds_tab <= (size_t)MI_LDS_MAX;          // (not at K = 32 with more than 256 source columns: counted in memory)
    const size_t lds1 = lds_row + (with_table ? lds_tab : 0);
    const size_t lds3 = lovasz_lds(p.npx_max, K).bytes();
    MI_REQUIRE(lds3 <= (size_t)MI_LDS_MAX, "mi_upsample_lovasz: upsample factor too large for one LDS tile (%zu B)", lds3);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(hist, 0, ((size_t)K * LOV_BINS * 2 + LOV_STATE) * sizeof(unsigned), st) != hipSuccess)
        return mi_set_error(MI_EHIP, "mi_upsample_lovasz: memset");
    with_kt(K, [&](auto kt) {
        constexpr auto kern = lovasz_count_kernel<decltype(kt)::value>;
        static std::atomic<uint64_t> lds_set;
        mi_allow_dynamic_lds((const void*)kern, MI_LDS_MAX, lds_set);
        hipLaunchKernelGGL(kern, dim3(pl.tiles_x, pl.row_groups, B), dim3(256), lds1, st, low, labels, hist, state, err, K, p.ay, p.ax, ignore_index, pl.rows,
                           ncol_max, with_table);
    });
    if (int rc = launch_failed("mi_upsample_lovasz", "count")) return rc;
    hipLaunchKernelGGL(lovasz_scan_kernel, dim3(K), dim3(256), 0, st, hist, state, coef);
    if (int rc = launch_failed("mi_upsample_lovasz", "scan")) return rc;
    with_kt(K, [&](auto kt) {
        launch_xtile<lovasz_grad_kernel<decltype(kt)::value>>(p, H, B, lds3, st, low, labels, (const float*)coef, (const unsigned*)state, partial, tmp, K, p.ay,
                                                              p.ax, ignore_index, p.npx_max, p.jt_cols);
    });
    if (int rc = launch_failed("mi_upsample_lovasz", "gradient")) return rc;
    hipLaunchKernelGGL(lovasz_finalize_kernel, dim3(1), dim3(256), 0, st, (const float*)partial, (long)B * H * p.tiles, (const unsigned*)state, loss_out);
    if (int rc = launch_failed("mi_upsample_lovasz", "finalize")) return rc;
    if (dlow) {
        hipLaunchKernelGGL(lovasz_pass2_kernel, dim3(nblk((long)B * h * w * K, 256)), dim3(256), 0, st, (const float*)tmp, dlow, B, K, p.ay, w, grad_scale);
        if (int rc = launch_failed("mi_upsample_lovasz", "gradient rows")) return rc;
    }
    if (hist_out && hipMemcpyAsync(hist_out, hist, (size_t)K * LOV_BINS * 2 * sizeof(unsigned), hipMemcpyDeviceToDevice, st) != hipSuccess)
        return mi_set_error(MI_EHIP, "mi_upsample_lovasz: copy of the counts");
    return MI_OK;
}
