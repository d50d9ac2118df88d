// The `aspp` input transform of a batch on the device (mi_augment_batch, include/mi355seg.h): ColorJitter, PIL's two-pass bicubic resize,
// pad / crop / mirror, ToTensor + Normalize, and the nearest-neighbour label path, equal to the PIL pipeline bit for bit.
//
// Five launches per batch whatever its size; blockIdx.y is the sample, blockIdx.x strides over that sample's work:
//   1 grey_sum   exact integer sum of the grey image as it stands when the contrast op runs (samples with a contrast op only)
//   2 jitter     the colour ops written once as a uint8 image, over the source rows / columns the output needs (hue costs fp64
//                divisions per pixel; every source pixel feeds ~4 taps of the horizontal pass, so it is not redone there)
//   3 hpass      horizontal bicubic pass over the needed rows and columns -> tmp (uint8 rounding is part of the result)
//   4 finish     vertical pass + pad / crop / mirror + /255, BGR255, (x - mean) / std through a 768-entry table per sample
//   5 label      nearest gather, id table, 255 fill, mirror
// uint8 rows are read as aligned dwords (a byte span is covered by the dwords around it and shifted into place) and written as dwords;
// single bytes only at image tails, padding borders and for the label gather.
//
// Arithmetic that decides bits is spelled with explicitly rounded operations and contraction is off: PIL's blend is fp32 without FMA, its
// HSV conversion mixes fp32 and fp64 (see rgb_to_hsv), Normalize is four separate fp32 roundings.
#include "mi_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int AUG_THREADS = 256;
constexpr int PRECISION_BITS = 22;      // PIL Resample.c

// One rounding each, never contracted (the pragma above covers this file's own expressions; the __f*_rn helpers of the HIP headers are
// plain operators compiled outside it, so they are not used here).
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

__device__ __forceinline__ int grey_of(const Px& p) { return (19595 * p.r + 38470 * p.g + 7471 * p.b + 0x8000) >> 16; }      // PIL L = ITU-R 601-2

// PIL ImageEnhance: Image.blend(degenerate, image, factor) on uint8, fp32, clipped
__device__ __forceinline__ int blend1(int deg, int v, float f) {
    const float t = f_add((float)deg, f_mul(f, (float)(v - deg)));
    return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

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

// ops [0, n) of the sample on one pixel; contrast_deg: int(mean(grey) + 0.5) of the image as it stood when the contrast op ran
__device__ __forceinline__ Px apply_ops(Px p, const MiAugSample& d, int n, int contrast_deg) {
    for (int k = 0; k < n; ++k) {
        const float f = d.factor[k];
        switch (d.op[k]) {
        case 1: p.r = blend1(0, p.r, f), p.g = blend1(0, p.g, f), p.b = blend1(0, p.b, f); break;
        case 2: p.r = blend1(contrast_deg, p.r, f), p.g = blend1(contrast_deg, p.g, f), p.b = blend1(contrast_deg, p.b, f); break;
        case 3: {
            const int gr = grey_of(p);
            p.r = blend1(gr, p.r, f), p.g = blend1(gr, p.g, f), p.b = blend1(gr, p.b, f);
            break;
        }
        case 4: {
            int H, S, V;
            rgb_to_hsv(p, H, S, V);
            p = hsv_to_rgb((H + d.hue_shift) & 255, S, V);
            break;
        }
        default: break;
        }
    }
    return p;
}

__device__ __forceinline__ int contrast_pos(const MiAugSample& d) {
    for (int k = 0; k < d.n_ops; ++k)
        if (d.op[k] == 2) return k;
    return -1;
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

__device__ __forceinline__ int contrast_degenerate(const MiAugSample& d) {
    // mean over the whole image in fp64 (sum / count), + 0.5, truncated: ImageStat.mean of the grey image, as ImageEnhance.Contrast does
    return (int)d_add((double)d.grey_sum / (double)((long long)d.H * d.W), 0.5);
}

// ---- 1: grey sum -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AUG_THREADS) void aug_grey_sum_kernel(MiAugSample* table) {
    MiAugSample& d = table[blockIdx.y];
    const int cpos = contrast_pos(d);
    if (cpos < 0) return;
    const long npix = (long)d.H * d.W, ngroups = (npix + 3) >> 2;
    unsigned long long acc = 0;
    for (long g = blockIdx.x * (long)AUG_THREADS + threadIdx.x; g < ngroups; g += (long)gridDim.x * AUG_THREADS) {
        Px px[4];
        const long p0 = g * 4;
        const int n = (int)min(4L, npix - p0);
        if (n == 4) {
            const uint32_t* q = reinterpret_cast<const uint32_t*>(d.img + p0 * 3);
            const uint32_t w[3] = {q[0], q[1], q[2]};
            unpack4(w, px);
        } else {
            for (int i = 0; i < n; ++i) px[i].r = d.img[(p0 + i) * 3], px[i].g = d.img[(p0 + i) * 3 + 1], px[i].b = d.img[(p0 + i) * 3 + 2];
        }
        for (int i = 0; i < n; ++i) acc += (unsigned)grey_of(apply_ops(px[i], d, cpos, 0));
    }
    // integer additions: any order gives the same sum
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    __shared__ unsigned long long part[AUG_THREADS / 64];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        for (int i = 0; i < AUG_THREADS / 64; ++i) s += part[i];
        atomicAdd(&d.grey_sum, s);
    }
}

// ---- 2: jitter -------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AUG_THREADS) void aug_jitter_kernel(const MiAugSample* table) {
    const MiAugSample& d = table[blockIdx.y];
    if (d.n_ops <= 0) return;
    const int deg = contrast_pos(d) >= 0 ? contrast_degenerate(d) : 0;
    const long npix = (long)d.H * d.W;
    const long g0 = ((long)d.ry0 * d.W) >> 2, g1 = ((long)d.ry1 * d.W + 3) >> 2;
    for (long g = g0 + blockIdx.x * (long)AUG_THREADS + threadIdx.x; g < g1; g += (long)gridDim.x * AUG_THREADS) {
        const long p0 = g * 4;
        const int col = (int)(p0 % d.W);
        if (col + 3 < d.W && (col >= d.rx1 || col + 3 < d.rx0)) continue;      // a group wholly outside the needed columns (and not wrapping to the next row)
        const int n = (int)min(4L, npix - p0);
        Px px[4];
        if (n == 4) {
            const uint32_t* q = reinterpret_cast<const uint32_t*>(d.img + p0 * 3);
            uint32_t w[3] = {q[0], q[1], q[2]};
            unpack4(w, px);
            for (int i = 0; i < 4; ++i) px[i] = apply_ops(px[i], d, d.n_ops, deg);
            pack4(px, w);
            uint32_t* o = reinterpret_cast<uint32_t*>(d.jit + p0 * 3);
            o[0] = w[0], o[1] = w[1], o[2] = w[2];
        } else {
            for (int i = 0; i < n; ++i) {
                Px p;
                p.r = d.img[(p0 + i) * 3], p.g = d.img[(p0 + i) * 3 + 1], p.b = d.img[(p0 + i) * 3 + 2];
                p = apply_ops(p, d, d.n_ops, deg);
                d.jit[(p0 + i) * 3] = (uint8_t)p.r, d.jit[(p0 + i) * 3 + 1] = (uint8_t)p.g, d.jit[(p0 + i) * 3 + 2] = (uint8_t)p.b;
            }
        }
    }
}

// ---- 3: horizontal pass ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AUG_THREADS) void aug_hpass_kernel(const MiAugSample* table) {
    const MiAugSample& d = table[blockIdx.y];
    if (d.hcoef == nullptr) return;
    const uint8_t* src = d.n_ops > 0 ? d.jit : d.img;
    const int tcols = d.cx1 - d.cx0, gpr = (tcols + 3) >> 2;
    const long items = (long)(d.ry1 - d.ry0) * gpr;
    for (long it = blockIdx.x * (long)AUG_THREADS + threadIdx.x; it < items; it += (long)gridDim.x * AUG_THREADS) {
        const int rr = (int)(it / gpr), gg = (int)(it % gpr);
        const uint8_t* row = src + (long)(d.ry0 + rr) * d.W * 3;
        Px out[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int x = d.cx0 + gg * 4 + i;
            out[i].r = out[i].g = out[i].b = 0;
            if (x >= d.cx1) continue;
            int x0 = d.hbound[2 * x], n = d.hbound[2 * x + 1];
            x0 = min(max(x0, 0), d.W);                       // a table can never steer a read out of the row
            n = min(min(n, d.hk), d.W - x0);
            const uintptr_t a = reinterpret_cast<uintptr_t>(row + (long)x0 * 3);
            const int s = (int)(a & 3), nb = 3 * n;
            const uint32_t* q = reinterpret_cast<const uint32_t*>(a - s);
            const int nd = (s + nb + 3) >> 2;
            int acc[3] = {1 << (PRECISION_BITS - 1), 1 << (PRECISION_BITS - 1), 1 << (PRECISION_BITS - 1)};
            int tap = 0, ch = 0, b = -s;
            int c = n > 0 ? d.hcoef[x] : 0;
            for (int w = 0; w < nd; ++w) {
                const uint32_t v = q[w];
#pragma unroll
                for (int k = 0; k < 4; ++k, ++b) {
                    if (b >= 0 && b < nb) {
                        acc[ch] += c * (int)((v >> (8 * k)) & 255u);
                        if (++ch == 3) {
                            ch = 0;
                            if (++tap < n) c = d.hcoef[(long)tap * d.sw + x];
                        }
                    }
                }
            }
            out[i].r = clip8(acc[0] >> PRECISION_BITS), out[i].g = clip8(acc[1] >> PRECISION_BITS), out[i].b = clip8(acc[2] >> PRECISION_BITS);
        }
        uint32_t w[3];
        pack4(out, w);
        uint32_t* o = reinterpret_cast<uint32_t*>(d.tmp + (long)rr * d.tstride + gg * 12);
        o[0] = w[0], o[1] = w[1], o[2] = w[2];
    }
}

// ---- 4: vertical pass, pad / crop / mirror, ToTensor + Normalize -------------------------------------------------------------------------------
__global__ __launch_bounds__(AUG_THREADS) void aug_finish_kernel(const MiAugSample* table, float* out_img, int oh, int ow) {
    const MiAugSample& d = table[blockIdx.y];
    __shared__ float lut[3][256];
    for (int i = threadIdx.x; i < 768; i += AUG_THREADS) {
        const int c = i >> 8, u = i & 255;          // c: output channel; mean / std are indexed by the output channel (Normalize runs after the reorder)
        const float x = d.to_bgr255 ? (float)u : f_div((float)u, 255.f);      // (u / 255) * 255 == u in fp32 for all 256 levels
        lut[c][u] = f_div(f_sub(x, d.mean[c]), d.std[c]);
    }
    __syncthreads();
    // where the vertical pass (or, without one, this kernel) reads: tmp, or the source itself when the horizontal pass is skipped
    const bool hp = d.hcoef != nullptr, vp = d.vcoef != nullptr;
    const uint8_t* src = hp ? d.tmp : (d.n_ops > 0 ? d.jit : d.img);
    const long stride = hp ? d.tstride : (long)d.W * 3;
    const int row0 = hp ? d.ry0 : 0, col0 = hp ? d.cx0 : 0, nrows = hp ? d.ry1 - d.ry0 : d.H;
    const int gpr = (ow + 3) >> 2;
    const long items = (long)oh * gpr;
    float* out = out_img + (long)blockIdx.y * 3 * oh * ow;
    const int c0 = d.to_bgr255 ? 2 : 0, c2 = 2 - c0;      // source channel of output channel 0 / 2
    for (long it = blockIdx.x * (long)AUG_THREADS + threadIdx.x; it < items; it += (long)gridDim.x * AUG_THREADS) {
        const int y = (int)(it / gpr), x4 = (int)(it % gpr) * 4;
        const int sy = y + d.off_y;
        const bool row_in = sy >= d.cy0 && sy < d.cy1;
        int xa = d.flip ? ow - 1 - (x4 + 3) : x4;             // lowest resampled column of the four (meaningful when the group is whole)
        xa += d.off_x;
        uint8_t u[4][3] = {};
        if (row_in) {
            int y0 = sy, nt = 1;
            if (vp) y0 = d.vbound[2 * sy], nt = min(d.vbound[2 * sy + 1], d.vk);
            if (x4 + 3 < ow && xa >= d.cx0 && xa + 3 < d.cx1) {
                int acc[12];
#pragma unroll
                for (int i = 0; i < 12; ++i) acc[i] = vp ? 1 << (PRECISION_BITS - 1) : 0;
                for (int t = 0; t < nt; ++t) {
                    const int r = min(max(y0 + t - row0, 0), nrows - 1);
                    const int c = vp ? d.vcoef[(long)t * d.sh + sy] : 1;
                    uint32_t w[3];
                    load_span12(src + r * stride + (long)(xa - col0) * 3, w);
#pragma unroll
                    for (int i = 0; i < 12; ++i) acc[i] += c * (int)((w[i >> 2] >> (8 * (i & 3))) & 255u);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int j = d.flip ? 3 - i : i;
#pragma unroll
                    for (int c = 0; c < 3; ++c) u[i][c] = (uint8_t)(vp ? clip8(acc[3 * j + c] >> PRECISION_BITS) : acc[3 * j + c]);
                }
            } else {
                for (int i = 0; i < 4; ++i) {
                    const int x = x4 + i;
                    if (x >= ow) break;
                    const int sx = (d.flip ? ow - 1 - x : x) + d.off_x;
                    if (sx < d.cx0 || sx >= d.cx1) continue;
                    int acc[3];
                    for (int c = 0; c < 3; ++c) acc[c] = vp ? 1 << (PRECISION_BITS - 1) : 0;
                    for (int t = 0; t < nt; ++t) {
                        const int r = min(max(y0 + t - row0, 0), nrows - 1);
                        const int cf = vp ? d.vcoef[(long)t * d.sh + sy] : 1;
                        const uint8_t* p = src + r * stride + (long)(sx - col0) * 3;
                        for (int c = 0; c < 3; ++c) acc[c] += cf * (int)p[c];
                    }
                    for (int c = 0; c < 3; ++c) u[i][c] = (uint8_t)(vp ? clip8(acc[c] >> PRECISION_BITS) : acc[c]);
                }
            }
        }
        float* o = out + (long)y * ow + x4;
        const long plane = (long)oh * ow;
        if (x4 + 3 < ow && (ow & 3) == 0) {
            *reinterpret_cast<f32x4*>(o) = f32x4{lut[0][u[0][c0]], lut[0][u[1][c0]], lut[0][u[2][c0]], lut[0][u[3][c0]]};
            *reinterpret_cast<f32x4*>(o + plane) = f32x4{lut[1][u[0][1]], lut[1][u[1][1]], lut[1][u[2][1]], lut[1][u[3][1]]};
            *reinterpret_cast<f32x4*>(o + 2 * plane) = f32x4{lut[2][u[0][c2]], lut[2][u[1][c2]], lut[2][u[2][c2]], lut[2][u[3][c2]]};
        } else {
            for (int i = 0; i < 4 && x4 + i < ow; ++i) {
                o[i] = lut[0][u[i][c0]];
                o[plane + i] = lut[1][u[i][1]];
                o[2 * plane + i] = lut[2][u[i][c2]];
            }
        }
    }
}

// ---- 5: label ----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AUG_THREADS) void aug_label_kernel(const MiAugSample* table, float* out_lab, int lh, int lw) {
    const MiAugSample& d = table[blockIdx.y];
    if (d.lab == nullptr) return;
    __shared__ float lut[256];
    for (int i = threadIdx.x; i < 256; i += AUG_THREADS) lut[i] = (float)d.lab_table[i];
    __syncthreads();
    // PIL NEAREST: source index int((x + 0.5) * in / out) in fp64, clamped
    const double fy = (double)d.H / (double)d.lab_sh, fx = (double)d.W / (double)d.lab_sw;
    const int gpr = (lw + 3) >> 2;
    const long items = (long)lh * gpr;
    float* out = out_lab + (long)blockIdx.y * lh * lw;
    for (long it = blockIdx.x * (long)AUG_THREADS + threadIdx.x; it < items; it += (long)gridDim.x * AUG_THREADS) {
        const int y = (int)(it / gpr), x4 = (int)(it % gpr) * 4;
        const int sy = y + d.off_y;
        const bool row_in = sy >= 0 && sy < d.lab_sh;
        const int iy = row_in ? min((int)d_mul((double)sy + 0.5, fy), d.H - 1) : 0;
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int x = x4 + i;
            const int sx = (d.flip ? lw - 1 - x : x) + d.off_x;
            v[i] = 255.f;
            if (x < lw && row_in && sx >= 0 && sx < d.lab_sw) {
                const int ix = min((int)d_mul((double)sx + 0.5, fx), d.W - 1);
                v[i] = lut[d.lab[(long)iy * d.W + ix]];
            }
        }
        float* o = out + (long)y * lw + x4;
        if (x4 + 3 < lw && (lw & 3) == 0) {
            *reinterpret_cast<f32x4*>(o) = f32x4{v[0], v[1], v[2], v[3]};
        } else {
            for (int i = 0; i < 4 && x4 + i < lw; ++i) o[i] = v[i];
        }
    }
}

int grid_x(long items) {
    const long b = (items + AUG_THREADS - 1) / AUG_THREADS;
    return (int)(b < 1 ? 1 : (b > 512 ? 512 : b));
}

}      // namespace

extern "C" int mi_augment_batch(void* table_dev, const void* table_host, int B, int out_h, int out_w, int lab_h, int lab_w, float* out_img,
                                float* out_lab, void* stream) {
    MI_REQUIRE(table_dev && table_host && out_img, "mi_augment_batch: null operand");
    MI_REQUIRE(B > 0 && B <= 65535 && out_h > 0 && out_w > 0, "mi_augment_batch: bad batch / output size (B=%d, %dx%d)", B, out_h, out_w);
    MI_REQUIRE(mi_aligned16(out_img) && (!out_lab || mi_aligned16(out_lab)), "mi_augment_batch: outputs must be 16-byte aligned");
    const MiAugSample* t = static_cast<const MiAugSample*>(table_host);
    long grey = 0, jit = 0, hp = 0, fin = (long)out_h * ((out_w + 3) / 4), labw = 0;
    for (int i = 0; i < B; ++i) {
        const MiAugSample& d = t[i];
        MI_REQUIRE(d.img && d.H > 0 && d.W > 0 && d.sh > 0 && d.sw > 0 && (reinterpret_cast<uintptr_t>(d.img) & 3) == 0, "mi_augment_batch: sample %d: image", i);
        MI_REQUIRE(d.grey_sum == 0, "mi_augment_batch: sample %d: grey_sum must be 0 on entry", i);
        MI_REQUIRE(d.n_ops >= 0 && d.n_ops <= 4, "mi_augment_batch: sample %d: n_ops %d", i, d.n_ops);
        int ncontrast = 0;
        for (int k = 0; k < d.n_ops; ++k) {
            MI_REQUIRE(d.op[k] >= 1 && d.op[k] <= 4, "mi_augment_batch: sample %d: op code %d", i, d.op[k]);
            ncontrast += d.op[k] == 2;
        }
        MI_REQUIRE(ncontrast <= 1, "mi_augment_batch: sample %d: more than one contrast op", i);
        MI_REQUIRE(d.n_ops == 0 || (d.jit && (reinterpret_cast<uintptr_t>(d.jit) & 3) == 0), "mi_augment_batch: sample %d: jit buffer", i);
        const bool hpass = d.sw != d.W, vpass = d.sh != d.H;
        MI_REQUIRE(hpass == (d.hcoef != nullptr) && hpass == (d.hbound != nullptr) && vpass == (d.vcoef != nullptr) && vpass == (d.vbound != nullptr),
                   "mi_augment_batch: sample %d: a pass has tables exactly when its size changes (%dx%d -> %dx%d)", i, d.H, d.W, d.sh, d.sw);
        MI_REQUIRE((!hpass || d.hk > 0) && (!vpass || d.vk > 0), "mi_augment_batch: sample %d: taps", i);
        // the window of the resampled image the output shows, and the source rows / columns it needs
        const int wy0 = d.off_y > 0 ? d.off_y : 0, wy1 = d.off_y + out_h < d.sh ? d.off_y + out_h : d.sh;
        const int wx0 = d.off_x > 0 ? d.off_x : 0, wx1 = d.off_x + out_w < d.sw ? d.off_x + out_w : d.sw;
        if (wy0 < wy1 && wx0 < wx1) {
            MI_REQUIRE(d.cy0 == wy0 && d.cy1 == wy1 && d.cx0 == wx0 && d.cx1 == wx1, "mi_augment_batch: sample %d: window [%d,%d)x[%d,%d) != [%d,%d)x[%d,%d)", i,
                       d.cy0, d.cy1, d.cx0, d.cx1, wy0, wy1, wx0, wx1);
        } else {
            MI_REQUIRE(d.cy0 >= d.cy1 || d.cx0 >= d.cx1, "mi_augment_batch: sample %d: the output shows nothing of the image but a window is given", i);
        }
        const bool empty = d.cy0 >= d.cy1 || d.cx0 >= d.cx1;
        if (!empty) {
            MI_REQUIRE(0 <= d.ry0 && d.ry0 < d.ry1 && d.ry1 <= d.H && 0 <= d.rx0 && d.rx0 < d.rx1 && d.rx1 <= d.W, "mi_augment_batch: sample %d: source window", i);
            MI_REQUIRE(vpass || (d.ry0 <= d.cy0 && d.cy1 <= d.ry1), "mi_augment_batch: sample %d: source rows do not cover the window", i);
            MI_REQUIRE(hpass || (d.rx0 <= d.cx0 && d.cx1 <= d.rx1), "mi_augment_batch: sample %d: source columns do not cover the window", i);
            if (hpass) {
                MI_REQUIRE(d.tmp && (reinterpret_cast<uintptr_t>(d.tmp) & 3) == 0 && d.tstride == 12 * ((d.cx1 - d.cx0 + 3) / 4), "mi_augment_batch: sample %d: tmp buffer / stride", i);
                hp = hp > (long)(d.ry1 - d.ry0) * (d.tstride / 12) ? hp : (long)(d.ry1 - d.ry0) * (d.tstride / 12);
            }
            if (d.n_ops > 0) jit = jit > ((long)(d.ry1 - d.ry0) * d.W + 3) / 4 ? jit : ((long)(d.ry1 - d.ry0) * d.W + 3) / 4;
        }
        if (ncontrast) grey = grey > ((long)d.H * d.W + 3) / 4 ? grey : ((long)d.H * d.W + 3) / 4;
        if (d.lab) {
            MI_REQUIRE(out_lab && lab_h > 0 && lab_w > 0 && d.lab_sh > 0 && d.lab_sw > 0, "mi_augment_batch: sample %d: label output", i);
            labw = (long)lab_h * ((lab_w + 3) / 4);
        }
        MI_REQUIRE(d.std[0] != 0.f && d.std[1] != 0.f && d.std[2] != 0.f, "mi_augment_batch: sample %d: std", i);
    }
    hipStream_t s = (hipStream_t)stream;
    MiAugSample* td = static_cast<MiAugSample*>(table_dev);
    if (grey) {
        hipLaunchKernelGGL(aug_grey_sum_kernel, dim3(grid_x(grey), B), dim3(AUG_THREADS), 0, s, td);
        MI_CHECK_LAUNCH("mi_augment_batch (grey sum)");
    }
    if (jit) {
        hipLaunchKernelGGL(aug_jitter_kernel, dim3(grid_x(jit), B), dim3(AUG_THREADS), 0, s, td);
        MI_CHECK_LAUNCH("mi_augment_batch (jitter)");
    }
    if (hp) {
        hipLaunchKernelGGL(aug_hpass_kernel, dim3(grid_x(hp), B), dim3(AUG_THREADS), 0, s, td);
        MI_CHECK_LAUNCH("mi_augment_batch (horizontal pass)");
    }
    hipLaunchKernelGGL(aug_finish_kernel, dim3(grid_x(fin), B), dim3(AUG_THREADS), 0, s, td, out_img, out_h, out_w);
    MI_CHECK_LAUNCH("mi_augment_batch (finish)");
    if (labw) {
        hipLaunchKernelGGL(aug_label_kernel, dim3(grid_x(labw), B), dim3(AUG_THREADS), 0, s, td, out_lab, lab_h, lab_w);
        MI_CHECK_LAUNCH("mi_augment_batch (label)");
    }
    return MI_OK;
}
