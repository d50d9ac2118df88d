// Surface-distance metrics of a batch of binary masks (mi_surface_score, TEST.SURFACE_METRICS): what the Hausdorff distance, its percentile, the
// average symmetric surface distance and surface Dice need, without the host ever seeing a distance map.  The definition (medpy's hd / hd95 /
// assd with connectivity 1, plus surface Dice), restated from include/mi355seg.h:
//   P = (pred == cls), G = (label == cls).  Surface S(M): the pixels of M with at least one of their four neighbours outside M; a neighbour
//   outside the image is outside M (M & ~binary_erosion(M, cross, border_value=0)).
//   d2(s) for s in S(P) = min over t in S(G) of (sx - tx)^2 + (sy - ty)^2, an exact integer; likewise from S(G) to S(P).
//   HD = sqrt(max d2 over both directions); HD-q = numpy's linear percentile of the CONCATENATION of both directed distance lists;
//   ASSD = the mean of the two directed mean distances; NSD(tau) = the share of surface pixels with d2 <= floor(tau^2).
//   Both masks empty: every distance 0, NSD 1.  Exactly one empty: undefined (flag 0, the distance fields 0).
// Integers everywhere except the two sums of sqrt(d2), and those use no floating-point atomics: two calls give the same bits.  Seven launches:
//   init      zeroes the accumulators and the two histograms
//   mark      one workgroup per row: the surface bits of both masks (left / right neighbours from the wave's ballot), one byte per pixel; counts
//   columns   one lane per column, lanes along x: a down sweep and an up sweep write g(x, y), the vertical distance to the nearest surface pixel
//             of the column, for both maps as one 32-bit word (0xffff: the column has no site; never squared)
//   rows      one workgroup per row, the row of g in LDS.  Only the surface pixels query: d2 = min over x' of (x - x')^2 + g(x', y)^2, scanning
//             x' outward from x until dx^2 >= best (from there on no site can lower the minimum, one at dx^2 == best included).  Overwrites the
//             row of g with d2 and the two surface flags; maxima, tolerance counts and the histogram of d2's high bits by integer atomics; the
//             sums of sqrt(d2) per thread -> wave xor butterfly -> one partial per row
//   select    one workgroup per image finds the high cells that hold the ranks floor r and floor r + 1
//   low       histograms the low bits of the d2 that fall into those two cells
//   finalize  the two order statistics, the fixed-order sum of the partials, and every output
#include "edt_common.h"

namespace {

typedef unsigned long long u64;

constexpr int SS_MAX_SIDE = EDT_MAX_SIDE;
constexpr int SS_MAX_T = MI_SURFACE_MAX_TOL;
constexpr int SS_D2_BITS = EDT_D2_BITS;
constexpr int SS_LOW_BITS = 12;              // the split of the two-level histogram: 8192 high cells of 4096 values each
constexpr int SS_LOW = 1 << SS_LOW_BITS;
constexpr int SS_HIGH = 1 << (SS_D2_BITS - SS_LOW_BITS);
constexpr long SS_MAX_GRID = 1l << 14;       // workgroups of a launch at most (64 per CU); beyond it a workgroup strides over the rows / columns
constexpr unsigned SS_D2_MASK = EDT_D2_MASK, SS_IS_P = 1u << 30, SS_IS_G = 1u << 31;
constexpr int SS_ACC = 24;                   // per image: |P|, |G|, |S(P)|, |S(G)|, the two maxima, [2 * t + direction] tolerance counts from 6
constexpr int SS_ACC_TOL = 6;
static_assert(MI_SURFACE_INTS == 11 + 2 * SS_MAX_T && SS_ACC >= SS_ACC_TOL + 2 * SS_MAX_T, "ints row: 11 fields, then 2 T tolerance counts");

struct SsTol {
    int n;
    int v[SS_MAX_T];
};

inline size_t ss_up(size_t n) { return (n + 255) & ~(size_t)255; }

struct SsWs {
    u64* acc;            // [B][SS_ACC]
    u64* sel;            // [B][4]: high cell and values below it, for rank floor r and for rank floor r + 1
    unsigned* hist1;     // [B][SS_HIGH]
    unsigned* hist2;     // [B][2][SS_LOW]
    double* partial;     // [B][H][2]
    unsigned* g;         // [B][H][W]
    uint8_t* surf;       // [B][H][W]
    size_t bytes;
};
inline SsWs ss_layout(void* base, int B, int H, int W) {
    SsWs w;
    const uintptr_t p = reinterpret_cast<uintptr_t>(base);      // integer arithmetic: the size query lays out from a null base
    size_t o = 0;
    const size_t px = (size_t)B * H * W;
    w.acc = reinterpret_cast<u64*>(p + o);
    o += ss_up((size_t)B * SS_ACC * sizeof(u64));
    w.sel = reinterpret_cast<u64*>(p + o);
    o += ss_up((size_t)B * 4 * sizeof(u64));
    w.hist1 = reinterpret_cast<unsigned*>(p + o);
    o += ss_up((size_t)B * SS_HIGH * sizeof(unsigned));
    w.hist2 = reinterpret_cast<unsigned*>(p + o);
    o += ss_up((size_t)B * 2 * SS_LOW * sizeof(unsigned));
    w.partial = reinterpret_cast<double*>(p + o);
    o += ss_up((size_t)B * H * 2 * sizeof(double));
    w.g = reinterpret_cast<unsigned*>(p + o);
    o += ss_up(px * sizeof(unsigned));
    w.surf = reinterpret_cast<uint8_t*>(p + o);
    o += ss_up(px);
    w.bytes = o;
    return w;
}

inline bool ss_sizes_ok(int B, int H, int W) { return B > 0 && H > 0 && W > 0 && B <= 65535 && H <= SS_MAX_SIDE && W <= SS_MAX_SIDE; }

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
    for (int m = 32; m > 0; m >>= 1) v += (unsigned)__shfl_xor((int)v, m);
    return v;
}
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
    for (int m = 32; m > 0; m >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, m));
    return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// `mult` (0, 1 or 2) values of cell `key` into a table of 32-bit counters in memory.  Two rounds of in-wave aggregation (the peel of
// polyp_score.hip): the lanes that hold the cell of the first lane still waiting retire, their leader adds their number; what is left adds
// one by one.  A clean contour has most of its d2 in a handful of cells.  Every lane of the wave calls.
__device__ __forceinline__ void ss_hist_add(unsigned* tab, unsigned key, unsigned mult, int lane) {
    unsigned add = mult;
    bool waiting = mult != 0u;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (waiting) {
            const unsigned k0 = (unsigned)__builtin_amdgcn_readfirstlane((int)key);
            const bool same = key == k0;
            const u64 m = __ballot(same), m2 = __ballot(same && mult == 2u);      // among the lanes still waiting
            if (same) {
                waiting = false;
                add = lane == __ffsll((long long)m) - 1 ? (unsigned)(__popcll(m) + __popcll(m2)) : 0u;
            }
        }
    }
    if (add) atomicAdd(&tab[key], add);
}

__global__ __launch_bounds__(256) void surface_init_kernel(u64* __restrict__ acc, unsigned* __restrict__ hist1, unsigned* __restrict__ hist2, int B) {
    const long n = (long)B * SS_HIGH;          // == B * 2 * SS_LOW
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        hist1[i] = 0u;
        hist2[i] = 0u;
        if (i < (long)B * SS_ACC) acc[i] = 0ull;
    }
}
static_assert(SS_HIGH == 2 * SS_LOW && SS_ACC <= SS_HIGH, "surface_init_kernel zeroes the three tables in one loop");

__global__ __launch_bounds__(256) void surface_mark_kernel(const uint8_t* __restrict__ pred, const long long* __restrict__ lab, int B, int H, int W, int cls,
                                                           uint8_t* __restrict__ surf, u64* __restrict__ acc) {
    __shared__ unsigned wcnt[4][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long rows = (long)B * H;
    for (long r = blockIdx.x; r < rows; r += gridDim.x) {              // one row per workgroup unless the grid is capped
        const int b = (int)(r / H), y = (int)(r % H);
        const long row0 = r * W;
        unsigned c_p = 0u, c_g = 0u, c_sp = 0u, c_sg = 0u;
        for (int x0 = 0; x0 < W; x0 += 256) {                          // uniform trip count: the ballots need every lane
            const int x = x0 + tid;
            const bool in = x < W;
            const long i = row0 + x;
            bool p = false, g = false, pu = false, pd = false, gu = false, gd = false;
            if (in) {
                p = pred[i] == cls;
                g = lab[i] == cls;
                if (y > 0) {
                    pu = pred[i - W] == cls;
                    gu = lab[i - W] == cls;
                }
                if (y < H - 1) {
                    pd = pred[i + W] == cls;
                    gd = lab[i + W] == cls;
                }
            }
            const u64 mp = __ballot(p), mg = __ballot(g);
            bool pl, pr, gl, gr;
            if (lane > 0) {
                pl = (mp >> (lane - 1)) & 1ull;
                gl = (mg >> (lane - 1)) & 1ull;
            } else {
                pl = in && x > 0 && pred[i - 1] == cls;
                gl = in && x > 0 && lab[i - 1] == cls;
            }
            if (lane < 63) {                                           // a lane beyond the row holds false: outside the image
                pr = (mp >> (lane + 1)) & 1ull;
                gr = (mg >> (lane + 1)) & 1ull;
            } else {
                pr = in && x + 1 < W && pred[i + 1] == cls;
                gr = in && x + 1 < W && lab[i + 1] == cls;
            }
            const bool sp = p && !(pu && pd && pl && pr), sg = g && !(gu && gd && gl && gr);
            if (in) surf[i] = (uint8_t)((sp ? 1 : 0) | (sg ? 2 : 0));
            c_p += p ? 1u : 0u;
            c_g += g ? 1u : 0u;
            c_sp += sp ? 1u : 0u;
            c_sg += sg ? 1u : 0u;
        }
        c_p = wave_sum_u32(c_p);
        c_g = wave_sum_u32(c_g);
        c_sp = wave_sum_u32(c_sp);
        c_sg = wave_sum_u32(c_sg);
        if (lane == 0) {
            wcnt[wave][0] = c_p;
            wcnt[wave][1] = c_g;
            wcnt[wave][2] = c_sp;
            wcnt[wave][3] = c_sg;
        }
        __syncthreads();
        if (tid < 4) {
            const unsigned v = wcnt[0][tid] + wcnt[1][tid] + wcnt[2][tid] + wcnt[3][tid];
            if (v) atomicAdd(&acc[(long)b * SS_ACC + tid], (u64)v);
        }
        __syncthreads();
    }
}

// g(x, y) of both maps (edt_sweep_column): bit 0 of a byte of `surf` is a surface pixel of P, bit 1 one of G.
__global__ __launch_bounds__(256) void surface_cols_kernel(const uint8_t* __restrict__ surf, unsigned* __restrict__ g, int B, int H, int W) {
    const long cols = (long)B * W;
    for (long c = (long)blockIdx.x * 256 + threadIdx.x; c < cols; c += (long)gridDim.x * 256) {
        const int b = (int)(c / W), x = (int)(c % W);
        const uint8_t* s = surf + (long)b * H * W + x;
        edt_sweep_column([=](int y) { return (unsigned)s[(long)y * W]; }, g + (long)b * H * W + x, H, W);
    }
}

__global__ __launch_bounds__(256) void surface_rows_kernel(unsigned* __restrict__ g, int B, int H, int W, SsTol tol, u64* __restrict__ acc,
                                                           unsigned* __restrict__ hist1, double* __restrict__ partial) {
    __shared__ unsigned row[SS_MAX_SIDE];
    __shared__ double wsum[4][2];
    __shared__ unsigned wmax[4][2];
    __shared__ unsigned wtol[4][2 * SS_MAX_T];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long rows = (long)B * H;
    for (long r = blockIdx.x; r < rows; r += gridDim.x) {
        const int b = (int)(r / H);
        const u64* a = acc + (long)b * SS_ACC;
        if (a[2] == 0ull || a[3] == 0ull) continue;                    // uniform: one mask empty (undefined) or both (nothing to measure)
        unsigned* grow = g + r * W;
        for (int x = tid; x < W; x += 256) row[x] = grow[x];
        __syncthreads();
        double s_p = 0.0, s_g = 0.0;
        unsigned m_p = 0u, m_g = 0u;
        unsigned tc[2 * SS_MAX_T];
#pragma unroll
        for (int t = 0; t < 2 * SS_MAX_T; ++t) tc[t] = 0u;
        for (int x0 = 0; x0 < W; x0 += 256) {
            const int x = x0 + tid;
            unsigned key = 0u, mult = 0u;
            if (x < W) {
                const unsigned v = row[x];
                unsigned word = 0u;
                if ((v & 0xffffu) == 0u) {                             // a surface pixel of P asks for the nearest surface pixel of G
                    const unsigned d = edt_query(row, x, W, 16);
                    s_p += __dsqrt_rn((double)d);
                    m_p = max(m_p, d);
#pragma unroll
                    for (int t = 0; t < SS_MAX_T; ++t)
                        if (t < tol.n && d <= (unsigned)tol.v[t]) ++tc[2 * t];
                    word = d | SS_IS_P;
                    key = d >> SS_LOW_BITS;
                    ++mult;
                }
                if ((v >> 16) == 0u) {
                    const unsigned d = edt_query(row, x, W, 0);
                    s_g += __dsqrt_rn((double)d);
                    m_g = max(m_g, d);
#pragma unroll
                    for (int t = 0; t < SS_MAX_T; ++t)
                        if (t < tol.n && d <= (unsigned)tol.v[t]) ++tc[2 * t + 1];
                    word |= d | SS_IS_G;                                // a pixel on both surfaces has d2 == 0 both ways: one field holds both
                    key = d >> SS_LOW_BITS;
                    ++mult;
                }
                grow[x] = word;
            }
            ss_hist_add(hist1 + (long)b * SS_HIGH, key, mult, lane);
        }
        // fixed order: xor butterfly in the wave, the four waves in wave order, one partial pair per row
        s_p = wave_sum_f64(s_p);
        s_g = wave_sum_f64(s_g);
        m_p = wave_max_u32(m_p);
        m_g = wave_max_u32(m_g);
#pragma unroll
        for (int t = 0; t < 2 * SS_MAX_T; ++t) tc[t] = wave_sum_u32(tc[t]);
        if (lane == 0) {
            wsum[wave][0] = s_p;
            wsum[wave][1] = s_g;
            wmax[wave][0] = m_p;
            wmax[wave][1] = m_g;
#pragma unroll
            for (int t = 0; t < 2 * SS_MAX_T; ++t) wtol[wave][t] = tc[t];
        }
        __syncthreads();
        if (tid < 2) {
            partial[r * 2 + tid] = ((wsum[0][tid] + wsum[1][tid]) + wsum[2][tid]) + wsum[3][tid];
            const unsigned m = max(max(wmax[0][tid], wmax[1][tid]), max(wmax[2][tid], wmax[3][tid]));
            if (m) atomicMax(&acc[(long)b * SS_ACC + 4 + tid], (u64)m);
        } else if (tid >= 64 && tid < 64 + 2 * SS_MAX_T) {
            const int t = tid - 64;
            const unsigned v = wtol[0][t] + wtol[1][t] + wtol[2][t] + wtol[3][t];
            if (v) atomicAdd(&acc[(long)b * SS_ACC + SS_ACC_TOL + t], (u64)v);
        }
        __syncthreads();
    }
}

// The cells that hold rank ka of histogram ha and rank kb of histogram hb (`cells` 32-bit counters each, a multiple of 256), and the number of
// values below each cell: out[0..1] for ka, out[2..3] for kb.  Every thread of the workgroup calls; the ranks lie below the histograms' totals.
__device__ __forceinline__ void ss_find2(const unsigned* __restrict__ ha, const unsigned* __restrict__ hb, int cells, u64 ka, u64 kb,
                                         unsigned (*part)[256], u64* out) {
    const int tid = threadIdx.x, per = cells / 256;
    unsigned sa = 0u, sb = 0u;
    for (int i = 0; i < per; ++i) {
        sa += ha[tid * per + i];
        sb += hb[tid * per + i];
    }
    part[0][tid] = sa;
    part[1][tid] = sb;
    __syncthreads();
    if (tid == 0 || tid == 64) {
        const int which = tid ? 1 : 0;
        const unsigned* h = which ? hb : ha;
        const u64 k = which ? kb : ka;
        u64 below = 0ull;
        int c = 0;
        while (c < 255 && below + part[which][c] <= k) below += part[which][c++];
        int i = c * per;
        const int last = i + per - 1;
        while (i < last && below + h[i] <= k) below += h[i++];
        out[2 * which] = (u64)i;
        out[2 * which + 1] = below;
    }
    __syncthreads();
}

struct SsRank {
    u64 n, fl, rem, k1;
    bool measured;
};
__device__ __forceinline__ SsRank ss_rank(const u64* a, int q_num) {
    SsRank r;
    r.n = a[2] + a[3];
    r.measured = a[2] != 0ull && a[3] != 0ull;
    r.fl = r.rem = r.k1 = 0ull;
    if (r.measured) {
        const u64 t = (u64)q_num * (r.n - 1ull);
        r.fl = t / 100ull;
        r.rem = t % 100ull;
        r.k1 = min(r.fl + 1ull, r.n - 1ull);
    }
    return r;
}

__global__ __launch_bounds__(256) void surface_select_kernel(const u64* __restrict__ acc, const unsigned* __restrict__ hist1, int q_num, u64* __restrict__ sel) {
    __shared__ unsigned part[2][256];
    __shared__ u64 found[4];
    const int b = blockIdx.x;
    const SsRank rk = ss_rank(acc + (long)b * SS_ACC, q_num);
    if (!rk.measured) return;                                          // uniform
    const unsigned* h = hist1 + (long)b * SS_HIGH;
    ss_find2(h, h, SS_HIGH, rk.fl, rk.k1, part, found);
    if (threadIdx.x < 4) sel[(long)b * 4 + threadIdx.x] = found[threadIdx.x];
}

__global__ __launch_bounds__(256) void surface_low_kernel(const unsigned* __restrict__ g, int B, int H, int W, const u64* __restrict__ acc,
                                                          const u64* __restrict__ sel, unsigned* __restrict__ hist2) {
    const int tid = threadIdx.x, lane = tid & 63;
    const long rows = (long)B * H;
    for (long r = blockIdx.x; r < rows; r += gridDim.x) {
        const int b = (int)(r / H);
        const u64* a = acc + (long)b * SS_ACC;
        if (a[2] == 0ull || a[3] == 0ull) continue;                    // the rows kernel wrote nothing here
        const unsigned c0 = (unsigned)sel[(long)b * 4], c1 = (unsigned)sel[(long)b * 4 + 2];
        unsigned* h0 = hist2 + (long)b * 2 * SS_LOW;
        for (int x0 = 0; x0 < W; x0 += 256) {
            const int x = x0 + tid;
            unsigned low = 0u, mult = 0u, cell = 0u;
            if (x < W) {
                const unsigned v = g[r * W + x];
                mult = (v >> 30 & 1u) + (v >> 31);
                const unsigned d = v & SS_D2_MASK;
                low = d & (SS_LOW - 1);
                cell = d >> SS_LOW_BITS;
            }
            ss_hist_add(h0, low, cell == c0 ? mult : 0u, lane);
            ss_hist_add(h0 + SS_LOW, low, cell == c1 ? mult : 0u, lane);
        }
    }
}

__global__ __launch_bounds__(256) void surface_finalize_kernel(int H, int q_num, int T, const u64* __restrict__ acc, const u64* __restrict__ sel,
                                                               const unsigned* __restrict__ hist2, const double* __restrict__ partial,
                                                               long long* __restrict__ ints, double* __restrict__ sums) {
    __shared__ unsigned part[2][256];
    __shared__ u64 found[4];
    __shared__ double wred[4][2];
    const int b = blockIdx.x, tid = threadIdx.x;
    const u64* a = acc + (long)b * SS_ACC;
    const SsRank rk = ss_rank(a, q_num);
    u64 lo = 0ull, hi = 0ull;
    double s0 = 0.0, s1 = 0.0;
    if (rk.measured) {                                                 // uniform
        const u64* sl = sel + (long)b * 4;
        const unsigned* h0 = hist2 + (long)b * 2 * SS_LOW;
        ss_find2(h0, h0 + SS_LOW, SS_LOW, rk.fl - sl[1], rk.k1 - sl[3], part, found);
        lo = (sl[0] << SS_LOW_BITS) | found[0];
        hi = (sl[2] << SS_LOW_BITS) | found[2];
        // thread t adds the rows t, t + 256, ... in ascending order, then the butterfly and the four waves in wave order
        for (int y = tid; y < H; y += 256) {
            s0 += partial[((long)b * H + y) * 2];
            s1 += partial[((long)b * H + y) * 2 + 1];
        }
        s0 = wave_sum_f64(s0);
        s1 = wave_sum_f64(s1);
        if ((tid & 63) == 0) {
            wred[tid >> 6][0] = s0;
            wred[tid >> 6][1] = s1;
        }
        __syncthreads();
        s0 = ((wred[0][0] + wred[1][0]) + wred[2][0]) + wred[3][0];
        s1 = ((wred[0][1] + wred[1][1]) + wred[2][1]) + wred[3][1];
    }
    long long* out = ints + (long)b * MI_SURFACE_INTS;
    if (tid == 0) {
        for (int i = 0; i < 6; ++i) out[i] = (long long)a[i];
        out[6] = (long long)lo;
        out[7] = (long long)hi;
        out[8] = (long long)rk.fl;
        out[9] = (long long)rk.rem;
        out[10] = (a[2] == 0ull) == (a[3] == 0ull) ? 1ll : 0ll;
        sums[(long)b * 2] = s0;
        sums[(long)b * 2 + 1] = s1;
    }
    if (tid < 2 * SS_MAX_T) out[11 + tid] = tid < 2 * T ? (long long)a[SS_ACC_TOL + tid] : 0ll;
}

}  // namespace

extern "C" size_t mi_surface_score_workspace(int B, int H, int W) {
    if (!ss_sizes_ok(B, H, W)) return 0;
    return ss_layout(nullptr, B, H, W).bytes;
}

extern "C" int mi_surface_score(const uint8_t* pred, const int64_t* labels, int B, int H, int W, int cls, int q_num, const int32_t* tol2, int T,
                                int64_t* ints, double* sums, void* workspace, size_t workspace_bytes, void* stream) {
    MI_REQUIRE(pred && labels && ints && sums && workspace, "mi_surface_score: null operand");
    MI_REQUIRE(B > 0 && H > 0 && W > 0, "mi_surface_score: bad dimension (B %d, masks %d x %d)", B, H, W);
    MI_REQUIRE(B <= 65535 && H <= SS_MAX_SIDE && W <= SS_MAX_SIDE, "mi_surface_score: B %d, masks %d x %d beyond the limits (B <= 65535, sides <= %d)", B, H,
               W, SS_MAX_SIDE);
    MI_REQUIRE(cls >= 0 && cls <= 255, "mi_surface_score: cls %d lies outside 0..255", cls);
    MI_REQUIRE(q_num >= 1 && q_num <= 100, "mi_surface_score: percentile %d lies outside 1..100", q_num);
    MI_REQUIRE(T >= 0 && T <= SS_MAX_T, "mi_surface_score: %d tolerances lie outside 0..%d", T, SS_MAX_T);
    MI_REQUIRE(T == 0 || tol2, "mi_surface_score: null operand (tol2 with T %d)", T);
    SsTol tol;
    tol.n = T;
    for (int t = 0; t < SS_MAX_T; ++t) tol.v[t] = 0;
    for (int t = 0; t < T; ++t) {
        MI_REQUIRE(tol2[t] >= 0, "mi_surface_score: tol2[%d] = %d is negative", t, (int)tol2[t]);
        tol.v[t] = tol2[t];
    }
    MI_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "mi_surface_score: workspace must be 8-byte aligned");
    const SsWs w = ss_layout(workspace, B, H, W);
    if (workspace_bytes < w.bytes) return mi_set_error(MI_ENOMEM, "mi_surface_score: workspace too small (%zu < %zu bytes)", workspace_bytes, w.bytes);
    const long long* lab = reinterpret_cast<const long long*>(labels);
    hipStream_t s = (hipStream_t)stream;
    const long rows = (long)B * H, col_wgs = ((long)B * W + 255) / 256, init_wgs = ((long)B * SS_HIGH + 255) / 256;
    const dim3 row_grid((unsigned)(rows < SS_MAX_GRID ? rows : SS_MAX_GRID)), col_grid((unsigned)(col_wgs < SS_MAX_GRID ? col_wgs : SS_MAX_GRID));
    hipLaunchKernelGGL(surface_init_kernel, dim3((unsigned)(init_wgs < SS_MAX_GRID ? init_wgs : SS_MAX_GRID)), dim3(256), 0, s, w.acc, w.hist1, w.hist2, B);
    hipLaunchKernelGGL(surface_mark_kernel, row_grid, dim3(256), 0, s, pred, lab, B, H, W, cls, w.surf, w.acc);
    hipLaunchKernelGGL(surface_cols_kernel, col_grid, dim3(256), 0, s, w.surf, w.g, B, H, W);
    hipLaunchKernelGGL(surface_rows_kernel, row_grid, dim3(256), 0, s, w.g, B, H, W, tol, w.acc, w.hist1, w.partial);
    hipLaunchKernelGGL(surface_select_kernel, dim3(B), dim3(256), 0, s, w.acc, w.hist1, q_num, w.sel);
    hipLaunchKernelGGL(surface_low_kernel, row_grid, dim3(256), 0, s, w.g, B, H, W, w.acc, w.sel, w.hist2);
    hipLaunchKernelGGL(surface_finalize_kernel, dim3(B), dim3(256), 0, s, H, q_num, T, w.acc, w.sel, w.hist2, w.partial, reinterpret_cast<long long*>(ints),
                       sums);
    MI_CHECK_LAUNCH("mi_surface_score");
    return MI_OK;
}
