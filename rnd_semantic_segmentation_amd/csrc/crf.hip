// Locally connected CRF refinement of the evaluation tail's probability map (mi_crf_refine; the definition: include/mi355seg.h).  Mean field over a
// dilated window, Gaussian position and bilateral kernels, Potts compatibility (the form of ConvCRF); all arithmetic fp32, exact expf / logf.
//   init      Q^0 = softmax(log(max(p, eps))) per pixel, planar probs -> pixel-major Q ([B][H][W][Kpad], Kpad = K rounded up to 4: one 128-bit
//             access brings four classes); with iters == 0 it writes the requested outputs instead
//   iterate   one launch per mean-field iteration, Q ping-pongs between the two workspace buffers, the last launch writes the outputs
// The iteration kernel works on the DILATION LATTICE: a workgroup owns 32 x 8 pixels of one residue class (y mod d, x mod d).  Their neighbours
// (i + (dy, dx) d) lie on the same lattice, so in lattice coordinates every window is dense with a halo of window / 2 <= 5 whatever the dilation:
// the staged tile is (32 + 2R) x (8 + 2R) lattice pixels (38 x 14 at the defaults, 2.1 x the pixels it owns; a dense tile with the 12-pixel halo
// of the defaults would stage 3.4 x, and one with the 80-pixel halo of window 11 x dilation 16 does not fit the LDS at all).  The tile holds all
// Kpad classes of Q plus the three image channels: a neighbour's weight (one expf) is computed once and applied to every class chunk.
// LDS layout: Q pixel-major with a pixel stride of an ODD number of 16-byte slots (Kpad / 4, plus one when that is even): a ds_read_b128 lane
// group is 16 lanes of one tile row, consecutive pixels then start in 16 different slots mod 16 - conflict-free; the image is planar (ds_read_b32,
// consecutive lanes on consecutive banks).  The d x d residue workgroups of one region read the same cache lines of Q and write the same lines of the
// output: the block index is decoded so that they follow each other on ONE XCD (blocks b and b + 8 share an XCD's L2).
// in(i, o) - the neighbour lies in the image - is one test for tile edges, image borders and halos beyond the image: a pixel outside the image is
// staged as zeros and its weight is zero.  Fixed neighbour order (row-major), no atomics: the same bits every call.
#include "mi_common.h"
#include <cmath>

namespace {

constexpr int CRF_TW = 32, CRF_TH = 8;       // lattice pixels a workgroup owns: one per thread, a wave = two tile rows
constexpr int CRF_THREADS = CRF_TW * CRF_TH;
constexpr int CRF_MAX_K = 32;
constexpr int CRF_MAX_WINDOW = 11;
constexpr int CRF_TAPS_PAD = 128;            // >= 11 x 11 table entries
constexpr int CRF_BATCH = 4;                 // global loads a thread has in flight while it stages the tile
constexpr float CRF_EPS = 1e-5f;

struct CrfParams {
    const float* probs;      // [B][K][H][W]
    const float* image;      // [B][3][H][W]
    const float* qin;        // [B][H][W][Kpad]
    float* qout;             // [B][H][W][Kpad] or NULL (last launch)
    float* out_probs;        // [B][K][H][W] or NULL
    uint8_t* pred;           // [B][H][W] or NULL
    float* conf;             // [B][H][W] or NULL
    int B, K, H, W, R, dil, tiles_x, tiles_y;
    long regions;            // B * tiles_y * tiles_x
    float cs0, cs1, cs2, pos_w, bi_w;
    float e_pos, e_bi, e_rgb;      // -1 / (2 sigma^2)
};

inline size_t crf_up256(size_t n) { return (n + 255) & ~(size_t)255; }
inline int crf_kpad(int K) { return (K + 3) & ~3; }
template <int NCH>
constexpr int crf_slots() { return NCH == 1 ? 1 : (NCH % 2 == 0 ? NCH + 1 : NCH); }

// softmax over v[0 .. K) in registers, then either the next Q (pixel-major, padding classes 0) or the requested outputs of pixel `pix` of image b.
template <int NCH>
__device__ __forceinline__ void crf_finish(float (&v)[NCH * 4], const CrfParams& p, int b, long pix) {
    constexpr int KP = NCH * 4;
    const int K = p.K;
    float m = v[0];
#pragma unroll
    for (int c = 1; c < KP; ++c)
        if (c < K) m = fmaxf(m, v[c]);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < KP; ++c) {
        v[c] = c < K ? expf(v[c] - m) : 0.f;
        s += v[c];
    }
#pragma unroll
    for (int c = 0; c < KP; ++c) v[c] = v[c] / s;
    const long plane = (long)p.H * p.W;
    if (p.qout) {
        float4* q = reinterpret_cast<float4*>(p.qout + ((long)b * plane + pix) * KP);
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) q[ch] = make_float4(v[4 * ch], v[4 * ch + 1], v[4 * ch + 2], v[4 * ch + 3]);
        return;
    }
    if (p.out_probs) {
        float* o = p.out_probs + (long)b * K * plane + pix;
#pragma unroll
        for (int c = 0; c < KP; ++c)
            if (c < K) o[(long)c * plane] = v[c];
    }
    if (p.pred || p.conf) {
        float best = v[0];
        int arg = 0;
#pragma unroll
        for (int c = 1; c < KP; ++c)
            if (c < K && v[c] > best) {      // strict: the lowest index among the maxima
                best = v[c];
                arg = c;
            }
        if (p.pred) p.pred[(long)b * plane + pix] = (uint8_t)arg;
        if (p.conf) p.conf[(long)b * plane + pix] = best;
    }
}

template <int NCH>
__device__ __forceinline__ void crf_unary(float (&v)[NCH * 4], const CrfParams& p, int b, long pix) {
    const long plane = (long)p.H * p.W;
    const float* src = p.probs + (long)b * p.K * plane + pix;
#pragma unroll
    for (int c = 0; c < NCH * 4; ++c) v[c] = c < p.K ? logf(fmaxf(src[(long)c * plane], CRF_EPS)) : 0.f;
}

template <int NCH>
__global__ __launch_bounds__(CRF_THREADS) void crf_init_kernel(CrfParams p) {
    const long plane = (long)p.H * p.W;
    const long i = (long)blockIdx.x * CRF_THREADS + threadIdx.x;
    if (i >= (long)p.B * plane) return;
    const int b = (int)(i / plane);
    const long pix = i - (long)b * plane;
    float v[NCH * 4];
    crf_unary<NCH>(v, p, b, pix);
    crf_finish<NCH>(v, p, b, pix);
}

template <int NCH>
__global__ __launch_bounds__(CRF_THREADS) void crf_iter_kernel(CrfParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char crf_lds[];
    constexpr int S = crf_slots<NCH>();
    constexpr int KP = NCH * 4;
    const int tid = threadIdx.x;
    const int R = p.R, d = p.dil, H = p.H, W = p.W;
    const int win = 2 * R + 1, TWh = CRF_TW + 2 * R, THh = CRF_TH + 2 * R, npx = TWh * THh;
    float4* qt = reinterpret_cast<float4*>(crf_lds);             // [npx][S]
    float* it = reinterpret_cast<float*>(qt + (long)npx * S);    // [3][npx]
    float* gpt = it + 3 * npx;                                   // [win * win], the centre included (unused)
    float* gbt = gpt + CRF_TAPS_PAD;

    // block -> (region, residue): the d * d residues of one region on consecutive slots of one XCD
    const long n = blockIdx.x;
    const int xcd = (int)(n & 7), dd = d * d;
    const long slot = n >> 3;
    const int res = (int)(slot % dd);
    const long rg = (slot / dd) * 8 + xcd;
    if (rg >= p.regions) return;
    const long tiles = (long)p.tiles_x * p.tiles_y;
    const int b = (int)(rg / tiles);
    const int t = (int)(rg - (long)b * tiles);
    const int ly0 = (t / p.tiles_x) * CRF_TH, lx0 = (t % p.tiles_x) * CRF_TW;
    const int ry = res / d, rx = res - ry * d;
    if ((long)ly0 * d + ry >= H || (long)lx0 * d + rx >= W) return;      // this residue's lattice ends before the tile (whole workgroup)

    const long plane = (long)H * W;
    const float4* qin = reinterpret_cast<const float4*>(p.qin) + (long)b * plane * NCH;
    const float* img = p.image + (long)b * 3 * plane;
    // staging in batches of CRF_BATCH loads per thread, all issued before the first LDS store: one round trip to memory per batch, not per load
    for (int base = tid; base < npx * NCH; base += CRF_THREADS * CRF_BATCH) {
        float4 q[CRF_BATCH];
        int dst[CRF_BATCH];
#pragma unroll
        for (int u = 0; u < CRF_BATCH; ++u) {
            const int i = base + u * CRF_THREADS;
            q[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            dst[u] = -1;
            if (i < npx * NCH) {
                const int px = i / NCH, ch = i - px * NCH;
                const int hy = px / TWh, hx = px - hy * TWh;
                const int gy = (ly0 - R + hy) * d + ry, gx = (lx0 - R + hx) * d + rx;      // negative lattice index -> negative pixel (ry, rx < d)
                dst[u] = px * S + ch;
                if ((unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) q[u] = qin[((long)gy * W + gx) * NCH + ch];
            }
        }
#pragma unroll
        for (int u = 0; u < CRF_BATCH; ++u)
            if (dst[u] >= 0) qt[dst[u]] = q[u];
    }
    for (int base = tid; base < 3 * npx; base += CRF_THREADS * CRF_BATCH) {
        float v[CRF_BATCH];
#pragma unroll
        for (int u = 0; u < CRF_BATCH; ++u) {
            const int i = base + u * CRF_THREADS;
            v[u] = 0.f;
            if (i < 3 * npx) {
                const int ch = i / npx, px = i - ch * npx;
                const int hy = px / TWh, hx = px - hy * TWh;
                const int gy = (ly0 - R + hy) * d + ry, gx = (lx0 - R + hx) * d + rx;
                if ((unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) v[u] = img[(long)ch * plane + (long)gy * W + gx];
            }
        }
#pragma unroll
        for (int u = 0; u < CRF_BATCH; ++u)
            if (base + u * CRF_THREADS < 3 * npx) it[base + u * CRF_THREADS] = v[u];
    }
    if (tid < win * win) {
        const int dy = tid / win - R, dx = tid % win - R;
        const float o2 = (float)((dy * dy + dx * dx) * dd);      // <= 50 * 256: exact
        gpt[tid] = expf(o2 * p.e_pos);
        gbt[tid] = expf(o2 * p.e_bi);
    }
    __syncthreads();

    const int lxl = tid & (CRF_TW - 1), lyl = tid / CRF_TW;
    const int y = (ly0 + lyl) * d + ry, x = (lx0 + lxl) * d + rx;
    if (y >= H || x >= W) return;                                 // no barrier below
    // the normalisers: geometry only, the in-image taps in row-major order
    float Np = 0.f, Nb = 0.f;
    for (int dy = -R; dy <= R; ++dy) {
        const bool iny = (unsigned)(y + dy * d) < (unsigned)H;
        for (int dx = -R; dx <= R; ++dx) {
            if (dy == 0 && dx == 0) continue;
            if (iny && (unsigned)(x + dx * d) < (unsigned)W) {
                const int tap = (dy + R) * win + dx + R;
                Np += gpt[tap];
                Nb += gbt[tap];
            }
        }
    }
    const float wp = Np > 0.f ? p.pos_w / Np : 0.f, wb = Nb > 0.f ? p.bi_w / Nb : 0.f;      // a term whose N is 0 is 0

    const int c0 = (lyl + R) * TWh + lxl + R;
    const float i0 = it[c0], i1 = it[npx + c0], i2 = it[2 * npx + c0];
    float acc[KP];
#pragma unroll
    for (int c = 0; c < KP; ++c) acc[c] = 0.f;
    for (int dy = -R; dy <= R; ++dy) {
        const bool iny = (unsigned)(y + dy * d) < (unsigned)H;
        for (int dx = -R; dx <= R; ++dx) {
            if (dy == 0 && dx == 0) continue;
            const int nb = c0 + dy * TWh + dx, tap = (dy + R) * win + dx + R;
            const float d0 = p.cs0 * (it[nb] - i0), d1 = p.cs1 * (it[npx + nb] - i1), d2 = p.cs2 * (it[2 * npx + nb] - i2);
            const float gc = expf((d0 * d0 + d1 * d1 + d2 * d2) * p.e_rgb);
            // in(i, o) as a factor, not a branch: everything it multiplies is finite (a pixel outside the image is staged as zeros)
            const float in = (iny && (unsigned)(x + dx * d) < (unsigned)W) ? 1.f : 0.f;
            const float k = in * (wp * gpt[tap] + wb * gbt[tap] * gc);
            const float4* q = qt + nb * S;
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) {
                const float4 v = q[ch];
                acc[4 * ch + 0] += k * v.x;
                acc[4 * ch + 1] += k * v.y;
                acc[4 * ch + 2] += k * v.z;
                acc[4 * ch + 3] += k * v.w;
            }
        }
    }
    const long pix = (long)y * W + x;
    float v[KP];
    crf_unary<NCH>(v, p, b, pix);
#pragma unroll
    for (int c = 0; c < KP; ++c) v[c] += acc[c];
    crf_finish<NCH>(v, p, b, pix);
}

inline size_t crf_lds_bytes(int nch, int R) {
    const int slots = nch == 1 ? 1 : (nch % 2 == 0 ? nch + 1 : nch);
    const size_t npx = (size_t)(CRF_TW + 2 * R) * (CRF_TH + 2 * R);
    return npx * slots * 16 + npx * 3 * 4 + 2 * CRF_TAPS_PAD * 4;
}

template <int NCH>
int crf_launch(CrfParams p, float* buf0, float* buf1, int iters, hipStream_t s) {
    static std::atomic<uint64_t> lds_allowed{0};
    const size_t lds = crf_lds_bytes(NCH, p.R);
    if (lds > 64 * 1024) mi_allow_dynamic_lds(reinterpret_cast<const void*>(&crf_iter_kernel<NCH>), MI_LDS_MAX, lds_allowed);
    float* const out_probs = p.out_probs;
    uint8_t* const pred = p.pred;
    float* const conf = p.conf;
    const long pixels = (long)p.B * p.H * p.W;
    const long groups = (p.regions + 7) / 8;
    const unsigned grid = (unsigned)(groups * 8 * p.dil * p.dil);
    // the outputs belong to the last launch only: every earlier one writes the next Q
    p.qin = nullptr;
    p.qout = iters > 0 ? buf0 : nullptr;
    if (iters > 0) p.out_probs = nullptr, p.pred = nullptr, p.conf = nullptr;
    hipLaunchKernelGGL(crf_init_kernel<NCH>, dim3((unsigned)((pixels + CRF_THREADS - 1) / CRF_THREADS)), dim3(CRF_THREADS), 0, s, p);
    for (int t = 0; t < iters; ++t) {
        const bool last = t == iters - 1;
        p.qin = (t & 1) ? buf1 : buf0;
        p.qout = last ? nullptr : ((t & 1) ? buf0 : buf1);
        if (last) p.out_probs = out_probs, p.pred = pred, p.conf = conf;
        hipLaunchKernelGGL(crf_iter_kernel<NCH>, dim3(grid), dim3(CRF_THREADS), lds, s, p);
    }
    MI_CHECK_LAUNCH("mi_crf_refine");
    return MI_OK;
}

inline bool crf_sigma_ok(float v) { return std::isfinite(v) && v > 0.f; }
inline bool crf_weight_ok(float v) { return std::isfinite(v) && v >= 0.f; }

}  // namespace

extern "C" size_t mi_crf_workspace(int B, int K, int H, int W) {
    if (B <= 0 || K <= 0 || K > CRF_MAX_K || H <= 0 || W <= 0) return 0;
    return 2 * crf_up256((size_t)B * (size_t)H * (size_t)W * (size_t)crf_kpad(K) * sizeof(float));
}

extern "C" int mi_crf_refine(const float* probs, const float* image, float cs0, float cs1, float cs2, float* out_probs, uint8_t* pred, float* conf, int B,
                             int K, int H, int W, int iters, int window, int dilation, float pos_w, float pos_xy, float bi_w, float bi_xy, float bi_rgb,
                             void* workspace, size_t workspace_bytes, void* stream) {
    MI_REQUIRE(probs && image, "mi_crf_refine: null operand");
    MI_REQUIRE(out_probs || pred || conf, "mi_crf_refine: no output requested (out_probs, pred and conf are all NULL)");
    MI_REQUIRE(B > 0 && H > 0 && W > 0, "mi_crf_refine: bad dimension (B %d, H %d, W %d)", B, H, W);
    MI_REQUIRE(K >= 1 && K <= CRF_MAX_K, "mi_crf_refine: K %d outside 1..%d", K, CRF_MAX_K);
    MI_REQUIRE(window >= 3 && window <= CRF_MAX_WINDOW && (window & 1), "mi_crf_refine: window %d must be odd and in 3..%d", window, CRF_MAX_WINDOW);
    MI_REQUIRE(dilation >= 1 && dilation <= 16, "mi_crf_refine: dilation %d outside 1..16", dilation);
    MI_REQUIRE(iters >= 0 && iters <= 32, "mi_crf_refine: iters %d outside 0..32", iters);
    MI_REQUIRE(crf_sigma_ok(pos_xy) && crf_sigma_ok(bi_xy) && crf_sigma_ok(bi_rgb), "mi_crf_refine: sigma must be positive and finite (pos_xy %g, bi_xy %g, bi_rgb %g)",
               (double)pos_xy, (double)bi_xy, (double)bi_rgb);
    MI_REQUIRE(crf_weight_ok(pos_w) && crf_weight_ok(bi_w), "mi_crf_refine: weight must be non-negative and finite (pos_w %g, bi_w %g)", (double)pos_w,
               (double)bi_w);
    MI_REQUIRE(std::isfinite(cs0) && std::isfinite(cs1) && std::isfinite(cs2), "mi_crf_refine: channel scale must be finite");
    MI_REQUIRE((long)B * H * W < (1l << 31), "mi_crf_refine: B * H * W must stay below 2^31");
    const size_t need = iters > 0 ? mi_crf_workspace(B, K, H, W) : 0;
    if (iters > 0) {
        MI_REQUIRE(workspace, "mi_crf_refine: null workspace");
        MI_REQUIRE(mi_aligned16(workspace), "mi_crf_refine: workspace must be 16-byte aligned");
        if (workspace_bytes < need) return mi_set_error(MI_ENOMEM, "mi_crf_refine: workspace too small (%zu < %zu bytes)", workspace_bytes, need);
    }
    CrfParams p;
    p.probs = probs;
    p.image = image;
    p.qin = nullptr;
    p.qout = nullptr;
    p.out_probs = out_probs;
    p.pred = pred;
    p.conf = conf;
    p.B = B, p.K = K, p.H = H, p.W = W, p.R = window / 2, p.dil = dilation;
    p.tiles_x = ((W + dilation - 1) / dilation + CRF_TW - 1) / CRF_TW;
    p.tiles_y = ((H + dilation - 1) / dilation + CRF_TH - 1) / CRF_TH;
    p.regions = (long)B * p.tiles_x * p.tiles_y;
    MI_REQUIRE((p.regions + 7) / 8 * 8 * dilation * dilation <= 0x7fffffffl, "mi_crf_refine: B * H * W beyond the index arithmetic (grid)");
    p.cs0 = cs0, p.cs1 = cs1, p.cs2 = cs2, p.pos_w = pos_w, p.bi_w = bi_w;
    p.e_pos = (float)(-1.0 / (2.0 * (double)pos_xy * (double)pos_xy));
    p.e_bi = (float)(-1.0 / (2.0 * (double)bi_xy * (double)bi_xy));
    p.e_rgb = (float)(-1.0 / (2.0 * (double)bi_rgb * (double)bi_rgb));
    float* buf0 = reinterpret_cast<float*>(workspace);
    float* buf1 = iters > 0 ? reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + need / 2) : nullptr;
    hipStream_t s = (hipStream_t)stream;
    switch ((K + 3) / 4) {
        case 1: return crf_launch<1>(p, buf0, buf1, iters, s);
        case 2: return crf_launch<2>(p, buf0, buf1, iters, s);
        case 3: return crf_launch<3>(p, buf0, buf1, iters, s);
        case 4: return crf_launch<4>(p, buf0, buf1, iters, s);
        case 5: return crf_launch<5>(p, buf0, buf1, iters, s);
        case 6: return crf_launch<6>(p, buf0, buf1, iters, s);
        case 7: return crf_launch<7>(p, buf0, buf1, iters, s);
        default: return crf_launch<8>(p, buf0, buf1, iters, s);
    }
}
