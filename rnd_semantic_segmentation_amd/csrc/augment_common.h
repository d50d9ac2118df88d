// What the input transforms on the device share (augment.hip: `aspp`, augment_pra.hip: `pra`): the explicitly rounded arithmetic, PIL's
// HSV pair, the dword span loads and packs of uint8 RGB rows, one output pixel of a fixed-point resampling pass along a row, and the
// per-sample ToTensor + Normalize table.
//
// Arithmetic that decides bits is spelled with explicitly rounded operations and contraction is off: PIL's blend is fp32 without FMA, its
// HSV conversion mixes fp32 and fp64 (see rgb_to_hsv), Normalize is four separate fp32 roundings.
#pragma once
#include "mi_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int AUG_THREADS = 256;
constexpr int PRECISION_BITS = 22;      // PIL Resample.c

// One rounding each, never contracted (the pragma above covers this header's and the including file's own expressions; the __f*_rn helpers
// of the HIP headers are plain operators compiled outside it, so they are not used here).
__device__ __forceinline__ float f_add(float a, float b) { return a + b; }
__device__ __forceinline__ float f_sub(float a, float b) { return a - b; }
__device__ __forceinline__ float f_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float f_div(float a, float b) { return a / b; }      // correctly rounded: hipcc's default for fp32 division
__device__ __forceinline__ double d_add(double a, double b) { return a + b; }
__device__ __forceinline__ double d_sub(double a, double b) { return a - b; }
__device__ __forceinline__ double d_mul(double a, double b) { return a * b; }

struct Px {
    int r, g, b;
};

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// PIL Convert.c rgb2hsv: s, rc, gc, bc and the r == max branch in fp32; the other two branches and the wrap into [0, 1) are evaluated in
// fp64 (the literals 2.0, 4.0, 6.0, 1.0 are doubles in C) and rounded to fp32; the scaling to uint8 in fp64.
__device__ __forceinline__ void rgb_to_hsv(const Px& p, int& H, int& S, int& V) {
    const int mx = max(p.r, max(p.g, p.b)), mn = min(p.r, min(p.g, p.b));
    V = mx;
    if (mx == mn) {
        H = 0;
        S = 0;
        return;
    }
    const float cr = (float)(mx - mn);
    const float s = f_div(cr, (float)mx);
    const float rc = f_div((float)(mx - p.r), cr), gc = f_div((float)(mx - p.g), cr), bc = f_div((float)(mx - p.b), cr);
    float h;
    if (p.r == mx)
        h = f_sub(bc, gc);
    else if (p.g == mx)
        h = (float)d_sub(d_add(2.0, (double)rc), (double)bc);
    else
        h = (float)d_sub(d_add(4.0, (double)gc), (double)rc);
    h = (float)fmod(d_add((double)h / 6.0, 1.0), 1.0);
    H = clip8((int)d_mul((double)h, 255.0));
    S = clip8((int)d_mul((double)s, 255.0));
}

// PIL Convert.c hsv2rgb: fp64 throughout, round half to even
__device__ __forceinline__ Px hsv_to_rgb(int H, int S, int V) {
    Px o;
    if (S == 0) {
        o.r = o.g = o.b = V;
        return o;
    }
    const double x = d_mul((double)H, 6.0) / 255.0;
    const double fi = floor(x);
    const double f = d_sub(x, fi);
    const double fs = (double)S / 255.0;
    const double v = (double)V;
    const int p = clip8((int)rint(d_mul(v, d_sub(1.0, fs))));
    const int q = clip8((int)rint(d_mul(v, d_sub(1.0, d_mul(fs, f)))));
    const int t = clip8((int)rint(d_mul(v, d_sub(1.0, d_mul(fs, d_sub(1.0, f))))));
    switch ((int)fi % 6) {
    case 0: o.r = V, o.g = t, o.b = p; break;
    case 1: o.r = q, o.g = V, o.b = p; break;
    case 2: o.r = p, o.g = V, o.b = t; break;
    case 3: o.r = p, o.g = q, o.b = V; break;
    case 4: o.r = t, o.g = p, o.b = V; break;
    default: o.r = V, o.g = p, o.b = q; break;
    }
    return o;
}

// four consecutive pixels (12 bytes, 4-byte aligned) <-> three dwords
__device__ __forceinline__ void unpack4(const uint32_t w[3], Px px[4]) {
    uint8_t b[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) b[i] = (w[i >> 2] >> (8 * (i & 3))) & 255u;
#pragma unroll
    for (int i = 0; i < 4; ++i) px[i].r = b[3 * i], px[i].g = b[3 * i + 1], px[i].b = b[3 * i + 2];
}
__device__ __forceinline__ void pack4(const Px px[4], uint32_t w[3]) {
    uint32_t b[12];
#pragma unroll
    for (int i = 0; i < 4; ++i) b[3 * i] = px[i].r, b[3 * i + 1] = px[i].g, b[3 * i + 2] = px[i].b;
#pragma unroll
    for (int i = 0; i < 3; ++i) w[i] = b[4 * i] | (b[4 * i + 1] << 8) | (b[4 * i + 2] << 16) | (b[4 * i + 3] << 24);
}

// 12 bytes from any address as three dwords: aligned loads of the dwords around them, shifted into place.  Reads at most up to the next
// 4-byte boundary after p + 12 (the buffers are readable to their size rounded up, mi355seg.h).
__device__ __forceinline__ void load_span12(const uint8_t* p, uint32_t w[3]) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const int s = (int)(a & 3);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(a - s);
    const uint32_t d0 = q[0], d1 = q[1], d2 = q[2];
    if (s == 0) {
        w[0] = d0, w[1] = d1, w[2] = d2;
        return;
    }
    const uint32_t d3 = q[3];
    const int sh = 8 * s;
    w[0] = (uint32_t)((((uint64_t)d1 << 32) | d0) >> sh);
    w[1] = (uint32_t)((((uint64_t)d2 << 32) | d1) >> sh);
    w[2] = (uint32_t)((((uint64_t)d3 << 32) | d2) >> sh);
}

// Output column x of one fixed-point resampling pass along an RGB row of `width` pixels: taps [x0, x0 + n) of the row weighted by
// coef[tap * cstride + x] (tap-major table, at most k taps), rounded to uint8 as PIL does between its passes.  The row is read as the
// aligned dwords that cover the taps; a table can never steer a read out of the row.
__device__ __forceinline__ Px resample_row_px(const uint8_t* row, int width, int x0, int n, int k, const int32_t* coef, long cstride, int x) {
    x0 = min(max(x0, 0), width);
    n = min(min(n, k), width - x0);
    const uintptr_t a = reinterpret_cast<uintptr_t>(row + (long)x0 * 3);
    const int s = (int)(a & 3), nb = 3 * n;
    const uint32_t* q = reinterpret_cast<const uint32_t*>(a - s);
    const int nd = (s + nb + 3) >> 2;
    int acc[3] = {1 << (PRECISION_BITS - 1), 1 << (PRECISION_BITS - 1), 1 << (PRECISION_BITS - 1)};
    int tap = 0, ch = 0, b = -s;
    int c = n > 0 ? coef[x] : 0;
    for (int w = 0; w < nd; ++w) {
        const uint32_t v = q[w];
#pragma unroll
        for (int j = 0; j < 4; ++j, ++b) {
            if (b >= 0 && b < nb) {
                acc[ch] += c * (int)((v >> (8 * j)) & 255u);
                if (++ch == 3) {
                    ch = 0;
                    if (++tap < n) c = coef[(long)tap * cstride + x];
                }
            }
        }
    }
    Px o;
    o.r = clip8(acc[0] >> PRECISION_BITS), o.g = clip8(acc[1] >> PRECISION_BITS), o.b = clip8(acc[2] >> PRECISION_BITS);
    return o;
}

// ToTensor + Normalize of one sample as a table over (output channel, grey level): /255 (or the level itself for BGR255), - mean, / std,
// each one fp32 rounding; mean / std are indexed by the output channel (Normalize runs after the reorder).  All threads of the block call it.
__device__ __forceinline__ void fill_normalise_table(float (*lut)[256], bool to_bgr255, const float* mean, const float* std) {
    for (int i = threadIdx.x; i < 768; i += AUG_THREADS) {
        const int c = i >> 8, u = i & 255;
        const float x = to_bgr255 ? (float)u : f_div((float)u, 255.f);      // (u / 255) * 255 == u in fp32 for all 256 levels
        lut[c][u] = f_div(f_sub(x, mean[c]), std[c]);
    }
    __syncthreads();
}

inline int grid_x(long items) {
    const long b = (items + AUG_THREADS - 1) / AUG_THREADS;
    return (int)(b < 1 ? 1 : (b > 512 ? 512 : b));
}

}      // namespace
