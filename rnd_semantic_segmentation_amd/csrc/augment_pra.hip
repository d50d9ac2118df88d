// The `pra` input transform of a batch on the device (mi_augment_pra_batch, include/mi355seg.h): one of the eight symmetries of the
// square, HueSaturationValue, RandomBrightnessContrast, a 220 x 220 window, PIL's two-pass bilinear resize, ToTensor + Normalize, and the
// nearest-neighbour mask path, equal to the PIL pipeline bit for bit.  The host plan (host/pra_augment.py) decides everything; the
// kernels execute it.
//
// Four launches per batch whatever its size; blockIdx.y is the sample, blockIdx.x strides over that sample's work:
//   1 gather   the window of the transformed frame, read through the symmetry, colour applied, written once as a contiguous uint8 image
//              (a transposed source is walked by columns here and nowhere else; the HSV pair costs fp64 divisions per pixel and every
//              pixel feeds several taps of the horizontal pass, so it is not redone there)
//   2 hpass    horizontal pass over the window -> tmp (uint8 rounding is part of the result)
//   3 finish   vertical pass + /255, (x - mean) / std through a 768-entry table per sample
//   4 mask     nearest gather through the same symmetry and window, and the 256-entry table
// Rows of win / tmp are padded to whole groups of four pixels (12 bytes), so they are read and written as dwords throughout; source rows
// are read as dword spans when the symmetry keeps them rows, as single bytes when it turns them into columns and at row tails.
#include "augment_common.h"

#pragma clang fp contract(off)

namespace {

// pixel (ty, tx) of the transformed frame -> (source row, source column)
__device__ __forceinline__ void source_of(const MiPraSample& d, int ty, int tx, int& sy, int& sx) {
    const int a = (d.sym & 4) ? tx : ty, b = (d.sym & 4) ? ty : tx;
    sy = (d.sym & 2) ? d.H - 1 - a : a;
    sx = (d.sym & 1) ? d.W - 1 - b : b;
}

__device__ __forceinline__ Px colour(Px p, const MiPraSample& d) {
    if (d.hsv) {
        int H, S, V;
        rgb_to_hsv(p, H, S, V);
        p = hsv_to_rgb((H + d.hue_shift) & 255, d.lut_s[S], d.lut_v[V]);
    }
    if (d.bc) p.r = d.lut_bc[p.r], p.g = d.lut_bc[p.g], p.b = d.lut_bc[p.b];
    return p;
}

// ---- 1: gather + colour ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AUG_THREADS) void pra_gather_kernel(const MiPraSample* table) {
    const MiPraSample& d = table[blockIdx.y];
    const int gpr = (d.ww + 3) >> 2;
    const long items = (long)d.wh * gpr;
    const bool rows = (d.sym & 4) == 0, mirrored = (d.sym & 1) != 0;
    for (long it = blockIdx.x * (long)AUG_THREADS + threadIdx.x; it < items; it += (long)gridDim.x * AUG_THREADS) {
        const int y = (int)(it / gpr), x4 = (int)(it % gpr) * 4;
        Px px[4];
        if (rows && x4 + 3 < d.ww) {
            // four neighbours of a source row, ascending or descending: one span
            int sy, sa, sb;
            source_of(d, d.y0 + y, d.x0 + x4, sy, sa);
            source_of(d, d.y0 + y, d.x0 + x4 + 3, sy, sb);
            uint32_t w[3];
            load_span12(d.img + ((long)sy * d.W + min(sa, sb)) * 3, w);
            Px t[4];
            unpack4(w, t);
#pragma unroll
            for (int i = 0; i < 4; ++i) px[i] = colour(t[mirrored ? 3 - i : i], d);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                px[i].r = px[i].g = px[i].b = 0;
                if (x4 + i >= d.ww) continue;
                int sy, sx;
                source_of(d, d.y0 + y, d.x0 + x4 + i, sy, sx);
                const uint8_t* p = d.img + ((long)sy * d.W + sx) * 3;
                px[i].r = p[0], px[i].g = p[1], px[i].b = p[2];
                px[i] = colour(px[i], d);
            }
        }
        uint32_t w[3];
        pack4(px, w);
        uint32_t* o = reinterpret_cast<uint32_t*>(d.win + (long)y * d.wstride + x4 * 3);
        o[0] = w[0], o[1] = w[1], o[2] = w[2];
    }
}

// ---- 2: horizontal pass ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AUG_THREADS) void pra_hpass_kernel(const MiPraSample* table, int ow) {
    const MiPraSample& d = table[blockIdx.y];
    if (d.hcoef == nullptr) return;
    const int gpr = (ow + 3) >> 2;
    const long items = (long)d.wh * gpr;
    for (long it = blockIdx.x * (long)AUG_THREADS + threadIdx.x; it < items; it += (long)gridDim.x * AUG_THREADS) {
        const int y = (int)(it / gpr), x4 = (int)(it % gpr) * 4;
        const uint8_t* row = d.win + (long)y * d.wstride;
        Px out[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int x = x4 + i;
            out[i].r = out[i].g = out[i].b = 0;
            if (x >= ow) continue;
            out[i] = resample_row_px(row, d.ww, d.hbound[2 * x], d.hbound[2 * x + 1], d.hk, d.hcoef, ow, x);
        }
        uint32_t w[3];
        pack4(out, w);
        uint32_t* o = reinterpret_cast<uint32_t*>(d.tmp + (long)y * d.tstride + x4 * 3);
        o[0] = w[0], o[1] = w[1], o[2] = w[2];
    }
}

// ---- 3: vertical pass, ToTensor + Normalize ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AUG_THREADS) void pra_finish_kernel(const MiPraSample* table, float* out_img, int oh, int ow) {
    const MiPraSample& d = table[blockIdx.y];
    __shared__ float lut[3][256];
    fill_normalise_table(lut, false, d.mean, d.std);
    const bool hp = d.hcoef != nullptr, vp = d.vcoef != nullptr;
    const uint8_t* src = hp ? d.tmp : d.win;
    const long stride = hp ? d.tstride : d.wstride;
    const int gpr = (ow + 3) >> 2;
    const long items = (long)oh * gpr, plane = (long)oh * ow;
    float* out = out_img + (long)blockIdx.y * 3 * plane;
    for (long it = blockIdx.x * (long)AUG_THREADS + threadIdx.x; it < items; it += (long)gridDim.x * AUG_THREADS) {
        const int y = (int)(it / gpr), x4 = (int)(it % gpr) * 4;
        int y0 = y, nt = 1;
        if (vp) y0 = d.vbound[2 * y], nt = min(d.vbound[2 * y + 1], d.vk);
        int acc[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) acc[i] = vp ? 1 << (PRECISION_BITS - 1) : 0;
        for (int t = 0; t < nt; ++t) {
            const int r = min(max(y0 + t, 0), d.wh - 1);                       // a table can never steer a read out of the window
            const int c = vp ? d.vcoef[(long)t * oh + y] : 1;
            const uint32_t* q = reinterpret_cast<const uint32_t*>(src + r * stride + x4 * 3);      // rows are padded to whole groups
            const uint32_t w[3] = {q[0], q[1], q[2]};
#pragma unroll
            for (int i = 0; i < 12; ++i) acc[i] += c * (int)((w[i >> 2] >> (8 * (i & 3))) & 255u);
        }
        uint8_t u[4][3];
#pragma unroll
        for (int i = 0; i < 12; ++i) u[i / 3][i % 3] = (uint8_t)(vp ? clip8(acc[i] >> PRECISION_BITS) : acc[i]);
        float* o = out + (long)y * ow + x4;
        if (x4 + 3 < ow && (ow & 3) == 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) *reinterpret_cast<f32x4*>(o + c * plane) = f32x4{lut[c][u[0][c]], lut[c][u[1][c]], lut[c][u[2][c]], lut[c][u[3][c]]};
        } else {
            for (int i = 0; i < 4 && x4 + i < ow; ++i)
                for (int c = 0; c < 3; ++c) o[c * plane + i] = lut[c][u[i][c]];
        }
    }
}

// ---- 4: mask ---------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AUG_THREADS) void pra_mask_kernel(const MiPraSample* table, float* out_mask, int oh, int ow) {
    const MiPraSample& d = table[blockIdx.y];
    if (d.mask == nullptr) return;
    __shared__ float lut[256];
    for (int i = threadIdx.x; i < 256; i += AUG_THREADS) lut[i] = (float)d.mask_table[i];
    __syncthreads();
    const int gpr = (ow + 3) >> 2;
    const long items = (long)oh * gpr;
    float* out = out_mask + (long)blockIdx.y * oh * ow;
    for (long it = blockIdx.x * (long)AUG_THREADS + threadIdx.x; it < items; it += (long)gridDim.x * AUG_THREADS) {
        const int y = (int)(it / gpr), x4 = (int)(it % gpr) * 4;
        const int wy = min(max(d.ny[y], 0), d.wh - 1);
        float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (x4 + i >= ow) continue;
            const int wx = min(max(d.nx[x4 + i], 0), d.ww - 1);
            int sy, sx;
            source_of(d, d.y0 + wy, d.x0 + wx, sy, sx);
            v[i] = lut[d.mask[(long)sy * d.W + sx]];
        }
        float* o = out + (long)y * ow + x4;
        if (x4 + 3 < ow && (ow & 3) == 0) {
            *reinterpret_cast<f32x4*>(o) = f32x4{v[0], v[1], v[2], v[3]};
        } else {
            for (int i = 0; i < 4 && x4 + i < ow; ++i) o[i] = v[i];
        }
    }
}

// taps of one PIL BILINEAR pass in -> out (Resample.c precompute_coeffs: support 1 scaled by max(in / out, 1))
int bilinear_taps(int in, int out) {
    const double scale = (double)in / (double)out;
    return (int)ceil(scale < 1.0 ? 1.0 : scale) * 2 + 1;
}

bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

}      // namespace

extern "C" int mi_augment_pra_batch(const void* table_dev, const void* table_host, int B, int out_h, int out_w, float* out_img, float* out_mask,
                                    void* stream) {
    MI_REQUIRE(table_dev && table_host && out_img, "mi_augment_pra_batch: null operand");
    MI_REQUIRE(B > 0 && B <= 65535 && out_h > 0 && out_w > 0, "mi_augment_pra_batch: bad batch / output size (B=%d, %dx%d)", B, out_h, out_w);
    MI_REQUIRE(mi_aligned16(out_img) && (!out_mask || mi_aligned16(out_mask)), "mi_augment_pra_batch: outputs must be 16-byte aligned");
    const MiPraSample* t = static_cast<const MiPraSample*>(table_host);
    const long fin = (long)out_h * ((out_w + 3) / 4);
    long gat = 0, hp = 0;
    bool any_mask = false;
    for (int i = 0; i < B; ++i) {
        const MiPraSample& d = t[i];
        MI_REQUIRE(d.img && aligned4(d.img) && d.H > 0 && d.W > 0, "mi_augment_pra_batch: sample %d: image", i);
        MI_REQUIRE(d.sym >= 0 && d.sym <= 7, "mi_augment_pra_batch: sample %d: symmetry %d", i, d.sym);
        const int th = (d.sym & 4) ? d.W : d.H, tw = (d.sym & 4) ? d.H : d.W;
        MI_REQUIRE(d.wh > 0 && d.ww > 0 && d.y0 >= 0 && d.x0 >= 0 && d.y0 <= th - d.wh && d.x0 <= tw - d.ww,
                   "mi_augment_pra_batch: sample %d: window [%d,+%d)x[%d,+%d) outside the transformed frame %dx%d", i, d.y0, d.wh, d.x0, d.ww, th, tw);
        MI_REQUIRE(d.win && aligned4(d.win) && d.wstride == 12 * ((d.ww + 3) / 4), "mi_augment_pra_batch: sample %d: win buffer / stride", i);
        const bool hpass = d.ww != out_w, vpass = d.wh != out_h;
        MI_REQUIRE(hpass == (d.hcoef != nullptr) && hpass == (d.hbound != nullptr) && vpass == (d.vcoef != nullptr) && vpass == (d.vbound != nullptr),
                   "mi_augment_pra_batch: sample %d: a pass has tables exactly when its size changes (%dx%d -> %dx%d)", i, d.wh, d.ww, out_h, out_w);
        MI_REQUIRE((!hpass || d.hk == bilinear_taps(d.ww, out_w)) && (!vpass || d.vk == bilinear_taps(d.wh, out_h)),
                   "mi_augment_pra_batch: sample %d: taps (%d, %d) are not the bilinear filter's for %dx%d -> %dx%d", i, d.hk, d.vk, d.wh, d.ww, out_h, out_w);
        if (hpass) {
            MI_REQUIRE(d.tmp && aligned4(d.tmp) && d.tstride == 12 * ((out_w + 3) / 4), "mi_augment_pra_batch: sample %d: tmp buffer / stride", i);
            hp = hp > (long)d.wh * (d.tstride / 12) ? hp : (long)d.wh * (d.tstride / 12);
        }
        MI_REQUIRE(d.hue_shift >= 0 && d.hue_shift <= 255, "mi_augment_pra_batch: sample %d: hue shift %d", i, d.hue_shift);
        if (d.mask) {
            MI_REQUIRE(out_mask && d.ny && d.nx, "mi_augment_pra_batch: sample %d: mask output / nearest tables", i);
            any_mask = true;
        }
        MI_REQUIRE(d.std[0] != 0.f && d.std[1] != 0.f && d.std[2] != 0.f, "mi_augment_pra_batch: sample %d: std", i);
        gat = gat > (long)d.wh * (d.wstride / 12) ? gat : (long)d.wh * (d.wstride / 12);
    }
    hipStream_t s = (hipStream_t)stream;
    const MiPraSample* td = static_cast<const MiPraSample*>(table_dev);
    hipLaunchKernelGGL(pra_gather_kernel, dim3(grid_x(gat), B), dim3(AUG_THREADS), 0, s, td);
    MI_CHECK_LAUNCH("mi_augment_pra_batch (gather)");
    if (hp) {
        hipLaunchKernelGGL(pra_hpass_kernel, dim3(grid_x(hp), B), dim3(AUG_THREADS), 0, s, td, out_w);
        MI_CHECK_LAUNCH("mi_augment_pra_batch (horizontal pass)");
    }
    hipLaunchKernelGGL(pra_finish_kernel, dim3(grid_x(fin), B), dim3(AUG_THREADS), 0, s, td, out_img, out_h, out_w);
    MI_CHECK_LAUNCH("mi_augment_pra_batch (finish)");
    if (any_mask) {
        hipLaunchKernelGGL(pra_mask_kernel, dim3(grid_x(fin), B), dim3(AUG_THREADS), 0, s, td, out_mask, out_h, out_w);
        MI_CHECK_LAUNCH("mi_augment_pra_batch (mask)");
    }
    return MI_OK;
}
