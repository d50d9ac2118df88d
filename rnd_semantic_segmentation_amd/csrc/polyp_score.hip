// The polyp evaluation tail (mi_polyp_score): PraNet's res2 map -> bilinear (align_corners False) to the label size -> sigmoid -> min-max over the
// batch -> per image the 2 x 256 histogram of the quantised probability split by ground truth, the per-quadrant moment sums of the S-measure, the
// label geometry, and optionally the normalised map and the tester's mask.  host/metrics.py (polyp_image_stats) turns these into Dice, IoU, F-beta,
// E-measure, S-measure and MAE.  All per-pixel arithmetic fp32, every sum of more than a wave's worth of terms in double.
//   scan      p = sigmoid(bilinear(low)) per pixel: batch min / max of p itself (no monotonicity argument needed: the scoring pass recomputes the
//             same bits with the same device function), G, the label column / row sums and the labels outside {0, 1}; integer atomics only
//   score     recomputes p, normalises, histogram in LDS (in-wave aggregation first), moment sums per thread in double -> wave butterfly -> one
//             partial row per workgroup in the workspace (no floating-point atomics anywhere)
//   finalize  fixed-order sum of the partial rows per image
// A workgroup owns PS_XT columns x `rows` rows of one image; a thread keeps one column (its x0 / x1 / lambda_x) and walks the rows.
#include "upsample_common.h"

namespace {

constexpr int PS_XT = 256;           // columns per workgroup: one per thread
constexpr int PS_MAX_ROWS = 32;      // rows a thread walks at most: its double accumulators meet at most 32 terms before the fixed-order tree
constexpr int PS_WG_TARGET = 2048;   // workgroups a launch aims for (8 per CU) before a workgroup takes more than one row
constexpr int PS_Q = 5;              // per quadrant: sum p, sum p^2, sum p g, sum p^2 g, G_q
constexpr int PS_NSUM = 4 * PS_Q;    // quadrants LT, RT, LB, RB
constexpr int PS_PEEL = 4;           // in-wave aggregation rounds: a near-binary map has (background, foreground) x (bin 0, bin 255) = 4 hot cells
constexpr int PS_BINS = 256;
constexpr int PS_MM_SLOTS = 64;      // min / max slots: a workgroup's atomicMin / atomicMax go to one of 64 addresses, a reader takes one per lane
static_assert(MI_POLYP_SUMS == PS_NSUM + 4, "sums row: 20 quadrant sums, cx, cy, min, max");

struct PsPlan {
    int tiles_x, rows, row_groups;
    long wgs;                        // workgroups per image
};
inline PsPlan ps_plan(int B, int H, int W) {
    PsPlan p;
    p.tiles_x = (W + PS_XT - 1) / PS_XT;
    const long units = (long)B * H * p.tiles_x;
    long rows = (units + PS_WG_TARGET - 1) / PS_WG_TARGET;
    p.rows = (int)(rows < 1 ? 1 : (rows > PS_MAX_ROWS ? PS_MAX_ROWS : rows));
    if (p.rows > H) p.rows = H;
    p.row_groups = (H + p.rows - 1) / p.rows;
    p.wgs = (long)p.row_groups * p.tiles_x;
    return p;
}

// The fp32 probability of one output pixel: a + l (b - a) along x, then along y (a constant map stays constant bit for bit, lambda 0 returns the
// source value), then 1 / (1 + exp(-z)).  Contraction is off: the scan and the scoring pass must compute the same bits.
__device__ __forceinline__ float ps_prob(const float* __restrict__ img, int w, int y0, int y1, float ly, int x0, int x1, float lx) {
#pragma clang fp contract(off)
    const float a = img[(long)y0 * w + x0], b = img[(long)y0 * w + x1];
    const float c = img[(long)y1 * w + x0], d = img[(long)y1 * w + x1];
    const float r0 = a + lx * (b - a);
    const float r1 = c + lx * (d - c);
    const float z = r0 + ly * (r1 - r0);
    return 1.f / (1.f + __expf(-z));
}

__device__ __forceinline__ float ps_normalise(float p, float mn, float den) {      // (p - min) / (max - min + 1e-8), den rounded once
#pragma clang fp contract(off)
    return (p - mn) / den;
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
    for (int m = 32; m > 0; m >>= 1) v += (unsigned long long)__shfl_xor((long long)v, m);
    return v;
}
__device__ __forceinline__ float wave_min(float v) {
    for (int m = 32; m > 0; m >>= 1) v = fminf(v, __shfl_xor(v, m));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
    for (int m = 32; m > 0; m >>= 1) v = fmaxf(v, __shfl_xor(v, m));
    return v;
}

// What both walking kernels know about their tile.
struct PsTile {
    int b, x, ya, yb, x0, x1;
    float lx;
    bool live;
};
__device__ __forceinline__ PsTile ps_tile(const Axis& ay, const Axis& ax, int rows, int tiles_x) {
    PsTile t;
    t.b = blockIdx.y;
    const int tile = blockIdx.x % tiles_x, rg = blockIdx.x / tiles_x;
    t.x = tile * PS_XT + threadIdx.x;
    t.live = t.x < ax.n_out;
    t.ya = rg * rows;
    t.yb = min(ay.n_out, t.ya + rows);
    t.x0 = t.x1 = 0;
    t.lx = 0.f;
    if (t.live) ax.src(t.x, t.x0, t.x1, t.lx);
    return t;
}

// minmax: [0 .. 63] the bits of the smallest p seen by the workgroups of a slot, [64 .. 127] of the largest (p >= 0: the unsigned order of the bits
// is the order of the values).  Measured with every workgroup on ONE pair of addresses, the scan of 1 x 352 x 352 took 19 us.
__global__ void polyp_init_kernel(unsigned long long* __restrict__ hist, unsigned long long* __restrict__ counts, unsigned* __restrict__ minmax, int B) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < (long)B * 2 * PS_BINS) hist[idx] = 0ull;
    if (idx < (long)B * MI_POLYP_COUNTS) counts[idx] = 0ull;
    if (idx < PS_MM_SLOTS) {
        minmax[idx] = __float_as_uint(2.f);
        minmax[PS_MM_SLOTS + idx] = 0u;
    }
}

// The batch's (min, max) of p from the slots: one slot per lane, butterfly; every lane of the calling wave gets the same pair.
__device__ __forceinline__ void ps_minmax(const unsigned* __restrict__ minmax, float& mn, float& mx) {
    const int lane = threadIdx.x & 63;
    mn = wave_min(__uint_as_float(minmax[lane]));
    mx = wave_max(__uint_as_float(minmax[PS_MM_SLOTS + lane]));
}

__global__ __launch_bounds__(256) void polyp_scan_kernel(const float* __restrict__ low, const long long* __restrict__ labels, Axis ay, Axis ax, int rows,
                                                         int tiles_x, unsigned* __restrict__ minmax, unsigned long long* __restrict__ counts) {
    __shared__ unsigned long long wcnt[4][MI_POLYP_COUNTS];
    __shared__ float wmm[4][2];
    const PsTile t = ps_tile(ay, ax, rows, tiles_x);
    const int W = ax.n_out, w = ax.n_in;
    const float* img = low + (long)t.b * ay.n_in * w;
    const long long* lab = labels + (long)t.b * ay.n_out * W;
    float mn = 2.f, mx = 0.f;
    unsigned cnt = 0u, bad = 0u;
    unsigned long long rs = 0ull;
    if (t.live) {
        for (int y = t.ya; y < t.yb; ++y) {
            int y0, y1;
            float ly;
            ay.src(y, y0, y1, ly);
            const float p = ps_prob(img, w, y0, y1, ly, t.x0, t.x1, t.lx);
            mn = fminf(mn, p);
            mx = fmaxf(mx, p);
            const long long g = lab[(long)y * W + t.x];
            if (g == 1) {
                ++cnt;
                rs += (unsigned long long)y;
            } else if (g != 0) {
                ++bad;
            }
        }
    }
    const unsigned long long c_g = wave_sum_u64(cnt), c_col = wave_sum_u64((unsigned long long)cnt * (unsigned long long)t.x), c_row = wave_sum_u64(rs),
                             c_bad = wave_sum_u64(bad);
    mn = wave_min(mn);
    mx = wave_max(mx);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        wcnt[wave][0] = c_g;
        wcnt[wave][1] = c_col;
        wcnt[wave][2] = c_row;
        wcnt[wave][3] = c_bad;
        wmm[wave][0] = mn;
        wmm[wave][1] = mx;
    }
    __syncthreads();
    if (threadIdx.x < MI_POLYP_COUNTS) {
        const unsigned long long v = wcnt[0][threadIdx.x] + wcnt[1][threadIdx.x] + wcnt[2][threadIdx.x] + wcnt[3][threadIdx.x];
        if (v) atomicAdd(&counts[(long)t.b * MI_POLYP_COUNTS + threadIdx.x], v);
    }
    if (threadIdx.x == 0) {          // integer min / max of the bits: the result does not depend on arrival order
        const int slot = (blockIdx.x + 7 * blockIdx.y) & (PS_MM_SLOTS - 1);
        atomicMin(&minmax[slot], __float_as_uint(fminf(fminf(wmm[0][0], wmm[1][0]), fminf(wmm[2][0], wmm[3][0]))));
        atomicMax(&minmax[PS_MM_SLOTS + slot], __float_as_uint(fmaxf(fmaxf(wmm[0][1], wmm[1][1]), fmaxf(wmm[2][1], wmm[3][1]))));
    }
}

// The split point of the S-measure's regions from the scan's integers: int(round_half_even(sum / G)) + 1 in double, as host/metrics.py computes it
// (one correctly rounded division and rint: the same double on both sides).  G == 0: no centroid, (0, 0) - the host takes the y == 0 branch.
__device__ __forceinline__ void ps_centre(const unsigned long long* __restrict__ cnt, int& cx, int& cy) {
    const unsigned long long G = cnt[0];
    cx = cy = 0;
    if (G) {
        cx = (int)rint((double)cnt[1] / (double)G) + 1;
        cy = (int)rint((double)cnt[2] / (double)G) + 1;
    }
}

// One pixel's cell into the workgroup's dense [2][256] table.  A trained net's map is nearly binary: most lanes of a wave hold one of four cells,
// and one LDS atomic per pixel would serialise there.  PS_PEEL rounds of in-wave aggregation (the peel of upsample_infer.hip's lds_hist_add): the
// lanes that hold the cell of the first lane still waiting retire, their leader adds their number.  What is left adds one by one.
__device__ __forceinline__ void ps_hist_add(unsigned* tab, unsigned key, bool live, int lane) {
    unsigned add = live ? 1u : 0u;
    bool waiting = live;
#pragma unroll
    for (int r = 0; r < PS_PEEL; ++r) {
        if (waiting) {
            const unsigned k0 = (unsigned)__builtin_amdgcn_readfirstlane((int)key);
            const bool same = key == k0;
            const unsigned long long m = __ballot(same);      // among the lanes still waiting
            if (same) {
                waiting = false;
                add = lane == __ffsll((long long)m) - 1 ? (unsigned)__popcll(m) : 0u;
            }
        }
    }
    if (add) atomicAdd(&tab[key], add);
}

// Rows [ya, yb) of the thread's column into acc (sum p, sum p^2, sum p g, sum p^2 g, G); every lane of the workgroup walks (the peel ballots).
__device__ __forceinline__ void ps_walk(const PsTile& t, int ya, int yb, const float* __restrict__ img, const long long* __restrict__ lab, const Axis& ay,
                                        int w, int W, float mn, float den, unsigned* tab, float* __restrict__ prob, uint8_t* __restrict__ pred,
                                        double (&acc)[PS_Q]) {
    for (int y = ya; y < yb; ++y) {
        unsigned key = 0u;
        if (t.live) {
            int y0, y1;
            float ly;
            ay.src(y, y0, y1, ly);
            const float pn = ps_normalise(ps_prob(img, w, y0, y1, ly, t.x0, t.x1, t.lx), mn, den);
            const long o = (long)y * W + t.x;
            const bool g = lab[o] == 1;
            if (prob) prob[o] = pn;
            if (pred) pred[o] = pn > 1.f - pn ? (uint8_t)1 : (uint8_t)0;
            const int q = min(PS_BINS - 1, max(0, (int)(pn * 255.f)));      // truncation; the clamps only keep a NaN in bounds
            key = (g ? PS_BINS : 0) + (unsigned)q;
            const double dp = (double)pn, dp2 = dp * dp;                     // exact: 24-bit squared
            acc[0] += dp;
            acc[1] += dp2;
            if (g) {
                acc[2] += dp;
                acc[3] += dp2;
                acc[4] += 1.0;
            }
        }
        ps_hist_add(tab, key, t.live, threadIdx.x & 63);
    }
}

__global__ __launch_bounds__(256) void polyp_score_kernel(const float* __restrict__ low, const long long* __restrict__ labels, Axis ay, Axis ax, int rows,
                                                          int tiles_x, const unsigned* __restrict__ minmax, const unsigned long long* __restrict__ counts,
                                                          unsigned long long* __restrict__ hist, double* __restrict__ partial, float* __restrict__ prob,
                                                          uint8_t* __restrict__ pred) {
    __shared__ unsigned tab[2 * PS_BINS];
    __shared__ double wred[4][PS_NSUM];
    const int tid = threadIdx.x;
    tab[tid] = 0u;
    tab[256 + tid] = 0u;
    __syncthreads();
    const PsTile t = ps_tile(ay, ax, rows, tiles_x);
    const int H = ay.n_out, W = ax.n_out, w = ax.n_in;
    const long plane = (long)t.b * H * W;
    float mn, mx, den;
    ps_minmax(minmax, mn, mx);
    {
#pragma clang fp contract(off)
        den = (mx - mn) + 1e-8f;
    }
    int cx, cy;
    ps_centre(counts + (long)t.b * MI_POLYP_COUNTS, cx, cy);
    const float* img = low + (long)t.b * ay.n_in * w;
    double top[PS_Q] = {0.0, 0.0, 0.0, 0.0, 0.0}, bot[PS_Q] = {0.0, 0.0, 0.0, 0.0, 0.0};
    float* pr = prob ? prob + plane : nullptr;
    uint8_t* pd = pred ? pred + plane : nullptr;
    ps_walk(t, t.ya, min(t.yb, cy), img, labels + plane, ay, w, W, mn, den, tab, pr, pd, top);        // rows above the split
    ps_walk(t, max(t.ya, cy), t.yb, img, labels + plane, ay, w, W, mn, den, tab, pr, pd, bot);        // rows from the split down
    // fixed order: xor butterfly in the wave, the four waves added in wave order, one partial row per workgroup
    const bool left = t.x < cx;
    const int wave = tid >> 6;
#pragma unroll
    for (int i = 0; i < PS_Q; ++i) {
        const double lt = wave_sum(left ? top[i] : 0.0), rt = wave_sum(left ? 0.0 : top[i]);
        const double lb = wave_sum(left ? bot[i] : 0.0), rb = wave_sum(left ? 0.0 : bot[i]);
        if ((tid & 63) == 0) {
            wred[wave][0 * PS_Q + i] = lt;
            wred[wave][1 * PS_Q + i] = rt;
            wred[wave][2 * PS_Q + i] = lb;
            wred[wave][3 * PS_Q + i] = rb;
        }
    }
    __syncthreads();                 // publishes wred and the table
    if (tid < PS_NSUM)
        partial[((long)t.b * gridDim.x + blockIdx.x) * PS_NSUM + tid] = ((wred[0][tid] + wred[1][tid]) + wred[2][tid]) + wred[3][tid];
    for (int c = tid; c < 2 * PS_BINS; c += 256) {
        const unsigned v = tab[c];
        if (v) atomicAdd(&hist[(long)t.b * 2 * PS_BINS + c], (unsigned long long)v);
    }
}

// sums[b]: the 20 quadrant sums - thread t adds the partial rows t, t + 256, ... in ascending order (20 independent loads per row: the first
// version, 12 threads per value walking the rows one load at a time, took 16 us for 704 rows and 36 us for 1 720), then the xor butterfly of
// the wave and the four waves in wave order - then cx, cy, and the batch's min / max of the unnormalised probability.
__global__ __launch_bounds__(256) void polyp_finalize_kernel(const double* __restrict__ partial, long wgs, const unsigned* __restrict__ minmax,
                                                             const unsigned long long* __restrict__ counts, double* __restrict__ sums) {
    __shared__ double wred[4][PS_NSUM];
    const int b = blockIdx.x, tid = threadIdx.x;
    double v[PS_NSUM];
#pragma unroll
    for (int k = 0; k < PS_NSUM; ++k) v[k] = 0.0;
    for (long i = tid; i < wgs; i += 256) {
        const double* row = partial + ((long)b * wgs + i) * PS_NSUM;
#pragma unroll
        for (int k = 0; k < PS_NSUM; ++k) v[k] += row[k];
    }
#pragma unroll
    for (int k = 0; k < PS_NSUM; ++k) {
        const double s = wave_sum(v[k]);
        if ((tid & 63) == 0) wred[tid >> 6][k] = s;
    }
    float mn, mx;
    ps_minmax(minmax, mn, mx);
    __syncthreads();
    double* out = sums + (long)b * MI_POLYP_SUMS;
    if (tid < PS_NSUM) out[tid] = ((wred[0][tid] + wred[1][tid]) + wred[2][tid]) + wred[3][tid];
    if (tid == 0) {
        int cx, cy;
        ps_centre(counts + (long)b * MI_POLYP_COUNTS, cx, cy);
        out[PS_NSUM + 0] = (double)cx;
        out[PS_NSUM + 1] = (double)cy;
        out[PS_NSUM + 2] = (double)mn;
        out[PS_NSUM + 3] = (double)mx;
    }
}

constexpr long PS_MAX_SIDE = 1l << 20;       // label rows / columns: the per-thread 32-bit label counts and x * count stay far from overflow
constexpr long PS_MAX_PIXELS = 1l << 40;     // B * H * W: 64-bit pixel offsets and integer sums exact in double
constexpr size_t PS_WS_HEAD = 2 * PS_MM_SLOTS * sizeof(unsigned);      // the min / max slots, then the partial rows

}  // namespace

extern "C" size_t mi_polyp_score_workspace(int B, int h, int w, int H, int W) {
    if (B <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return 0;
    const PsPlan p = ps_plan(B, H, W);
    return PS_WS_HEAD + up256((size_t)B * (size_t)p.wgs * PS_NSUM * sizeof(double));
}

extern "C" int mi_polyp_score(const float* low, const int64_t* labels, int B, int h, int w, int H, int W, int64_t* hist, double* sums, int64_t* counts,
                              float* prob, uint8_t* pred, void* workspace, size_t workspace_bytes, void* stream) {
    MI_REQUIRE(low && labels && hist && sums && counts && workspace, "mi_polyp_score: null operand");
    MI_REQUIRE(B > 0 && h > 0 && w > 0 && H > 0 && W > 0, "mi_polyp_score: bad dimension (B %d, map %d x %d, labels %d x %d)", B, h, w, H, W);
    MI_REQUIRE(B <= 65535 && H <= PS_MAX_SIDE && W <= PS_MAX_SIDE && (long)B * H * W <= PS_MAX_PIXELS && (long)B * h * w <= PS_MAX_PIXELS,
               "mi_polyp_score: B * H * W beyond the index arithmetic (B <= 65535, sides <= 2^20, pixels <= 2^40)");
    MI_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "mi_polyp_score: workspace must be 8-byte aligned");
    MI_REQUIRE(workspace_bytes >= mi_polyp_score_workspace(B, h, w, H, W), "mi_polyp_score: workspace too small (%zu < %zu bytes)", workspace_bytes,
               mi_polyp_score_workspace(B, h, w, H, W));
    const PsPlan p = ps_plan(B, H, W);
    MI_REQUIRE(p.wgs <= 0x7fffffffl, "mi_polyp_score: B * H * W beyond the index arithmetic (grid)");
    unsigned* minmax = reinterpret_cast<unsigned*>(workspace);
    double* partial = reinterpret_cast<double*>(reinterpret_cast<char*>(workspace) + PS_WS_HEAD);
    unsigned long long* hist_u = reinterpret_cast<unsigned long long*>(hist);
    unsigned long long* counts_u = reinterpret_cast<unsigned long long*>(counts);
    const long long* lab = reinterpret_cast<const long long*>(labels);
    const Axis ay = make_axis(h, H, 0), ax = make_axis(w, W, 0);
    const dim3 grid((unsigned)p.wgs, (unsigned)B);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(polyp_init_kernel, dim3(nblk((long)B * 2 * PS_BINS, 256)), dim3(256), 0, s, hist_u, counts_u, minmax, B);
    hipLaunchKernelGGL(polyp_scan_kernel, grid, dim3(256), 0, s, low, lab, ay, ax, p.rows, p.tiles_x, minmax, counts_u);
    hipLaunchKernelGGL(polyp_score_kernel, grid, dim3(256), 0, s, low, lab, ay, ax, p.rows, p.tiles_x, minmax, counts_u, hist_u, partial, prob, pred);
    hipLaunchKernelGGL(polyp_finalize_kernel, dim3(B), dim3(256), 0, s, partial, p.wgs, minmax, counts_u, sums);
    MI_CHECK_LAUNCH("mi_polyp_score");
    return MI_OK;
}
