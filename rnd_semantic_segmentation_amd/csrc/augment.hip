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
// Arithmetic that decides bits is spelled with explicitly rounded operations and contraction is off (augment_common.h, shared with the `pra`
// transform of augment_pra.hip).
#include "augment_common.h"

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ int grey_of(const Px& p) { return (19595 * p.r + 38470 * p.g + 7471 * p.b + 0x8000) >> 16; }      // PIL L = ITU-R 601-2

// PIL ImageEnhance: Image.blend(degenerate, image, factor) on uint8, fp32, clipped
__device__ __forceinline__ int blend1(int deg, int v, float f) {
    const float t = f_add((float)deg, f_mul(f, (float)(v - deg)));
    return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
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
            out[i] = resample_row_px(row, d.W, d.hbound[2 * x], d.hbound[2 * x + 1], d.hk, d.hcoef, d.sw, x);
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
    fill_normalise_table(lut, d.to_bgr255 != 0, d.mean, d.std);
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
