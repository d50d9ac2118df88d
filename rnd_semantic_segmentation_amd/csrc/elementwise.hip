// Small HBM-bound kernels: fused SGD step on flat buffers, ReLU-backward mask, FrozenBN fold, error plumbing.
#include "mi_common.h"
#include <mutex>
#include <stdlib.h>
#include <string.h>

static thread_local char g_err[512] = "";

int mi_set_error(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

const MiSwitches& mi_sw() {
    static MiSwitches sw;
    static std::once_flag once;
    std::call_once(once, [] {
        auto env = [](const char* name, int dflt) {
            const char* e = getenv(name);
            return e ? atoi(e) : dflt;
        };
        sw.igemm_staged = env("MI_IGEMM_STAGED", 1);
        sw.igemm_pp = env("MI_IGEMM_PP", 1);
        sw.igemm_pp_mink = env("MI_IGEMM_PP_MINK", 512);
        sw.igemm_mt = env("MI_IGEMM_MT", 0);
        sw.igemm_bn = env("MI_IGEMM_BN", 0);
        sw.igemm_pref = env("MI_IGEMM_PREF", 1);
        sw.pp_korder = env("MI_IGEMM_PP_KORDER", 1);
#ifdef MI_EXPERIMENTS
        sw.pp_loop = env("MI_IGEMM_PP_LOOP", 0);
#else
        sw.pp_loop = 0;
#endif
        sw.igemm_pw = env("MI_IGEMM_PW", 0);
        sw.wgrad_q3_slots = env("MI_WGRAD_Q3_SLOTS", 512);
        sw.wgrad_q3_slots_beside = env("MI_WGRAD_Q3_SLOTS_BESIDE", 448);
        sw.wgrad_s4_slots = env("MI_WGRAD_S4_SLOTS", 512);
        if (sw.wgrad_s4_slots < 64) sw.wgrad_s4_slots = 512;
        sw.wgrad_ti256 = env("MI_WGRAD_TI256", -1);
        sw.wgrad_p3 = env("MI_WGRAD_P3", 0);
        sw.wgrad_q3 = env("MI_WGRAD_Q3", 1);
        sw.wgrad_s4 = env("MI_WGRAD_S4", 1);
        sw.gconv_bn128 = env("MI_GCONV_BN128", 0);
        sw.gconv_kc = env("MI_GCONV_KC", 0);
        sw.gconv_remap = env("MI_GCONV_REMAP", 1);
        sw.gconv_ks2_wgs = env("MI_GCONV_KS2_WGS", 320);
        sw.gconv_kc32_wgs = env("MI_GCONV_KC32_WGS", 1536);
        sw.gconv_bn32_wgs = env("MI_GCONV_BN32_WGS", 256);
        sw.gconv_bn_any = env("MI_GCONV_BN_ANY", 1);
        sw.gconv_bn_c = env("MI_GCONV_BN_C", 64);
        sw.gconv_bn_force = env("MI_GCONV_BN_FORCE", 0);
        sw.gconv3_wgs = env("MI_GCONV3_WGS", 512);
#ifdef MI_EXPERIMENTS          // measurement switches: experiment builds only (the product library ignores the variables)
        sw.gconv_dbg = env("MI_GC_DBG", 0);
        sw.gw_dbg = env("MI_GW_DBG", 0);
#else
        sw.gconv_dbg = sw.gw_dbg = 0;
#endif
        sw.gwm_steps = env("MI_GWM_STEPS", 48);
        if (sw.gwm_steps < 1) sw.gwm_steps = 48;
        sw.gwm_fused3 = env("MI_GWM_FUSED3", 1);
        sw.gwgrad3 = env("MI_GWGRAD3", 1);
#ifdef MI_EXPERIMENTS
        sw.p3_dbg = env("MI_P3_DBG", 0);
#else
        sw.p3_dbg = 0;
#endif
        sw.pp_trace_wg = env("MI_PP_TRACE_WG", 0);
        sw.stem_direct = env("MI_STEM_DIRECT", 1);
        sw.stem_pool_wgrad = env("MI_STEM_POOL_WGRAD", 1);
        sw.head_mask = env("MI_HEAD_MASK", 1);
        sw.sgd_pack = env("MI_SGD_PACK", 1);
        sw.stem_wgrad_splits = env("MI_STEM_WGRAD_SPLITS", 512);
        if (sw.stem_wgrad_splits < 1 || sw.stem_wgrad_splits > 4096) sw.stem_wgrad_splits = 512;
    });
    return sw;
}

extern "C" int mi_version(void) { return MI355SEG_VERSION; }
extern "C" const char* mi_last_error(void) { return g_err; }

namespace {

// torch.optim.SGD (reference core/trainers/aspp_trainer.py:25-26,94-95): g' = g + wd*p; buf = mu*buf + g'; p -= lr*buf
__global__ void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, size_t n4, size_t n, float lr,
                           float mu, float wd) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        f32x4 pv = reinterpret_cast<f32x4*>(p)[i];
        const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
        f32x4 bv = reinterpret_cast<f32x4*>(buf)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float gg = gv[e] + wd * pv[e];
            bv[e] = mu * bv[e] + gg;
            pv[e] = pv[e] - lr * bv[e];
        }
        reinterpret_cast<f32x4*>(buf)[i] = bv;
        reinterpret_cast<f32x4*>(p)[i] = pv;
    }
    // tail (n % 4 elements) by the first threads of block 0
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const size_t i = (n4 << 2) + threadIdx.x;
        const float gg = g[i] + wd * p[i];
        const float b = mu * buf[i] + gg;
        buf[i] = b;
        p[i] = p[i] - lr * b;
    }
}

// the same update with the hyper-parameters read from device memory: a captured HIP graph replays with whatever learning rate
// the host wrote into `hyper` before the launch (a by-value kernel argument would be frozen into the graph)
__global__ void sgd_dev_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, size_t n4, size_t n,
                               const float* __restrict__ hyper) {
    const float lr = hyper[0], mu = hyper[1], wd = hyper[2];
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        f32x4 pv = reinterpret_cast<f32x4*>(p)[i];
        const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
        f32x4 bv = reinterpret_cast<f32x4*>(buf)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float gg = gv[e] + wd * pv[e];
            bv[e] = mu * bv[e] + gg;
            pv[e] = pv[e] - lr * bv[e];
        }
        reinterpret_cast<f32x4*>(buf)[i] = bv;
        reinterpret_cast<f32x4*>(p)[i] = pv;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const size_t i = (n4 << 2) + threadIdx.x;
        const float gg = g[i] + wd * p[i];
        const float b = mu * buf[i] + gg;
        buf[i] = b;
        p[i] = p[i] - lr * b;
    }
}

// ---- the SGD update and the bf16 repack of every conv weight in ONE pass (mi_sgd_step_pack) -------------------------------------------------
// pack_multi_kernel (pack_aspp.hip) re-reads every fp32 weight a moment after sgd_kernel wrote it.  Here a workgroup owns the same 32 (o) x 128 (i)
// group of one table row as there (same table, same first_block column), updates p / buf of each 32 x 32 tile with 16-byte accesses, keeps the new
// weights in LDS and writes both packed operands from there with 16-byte stores.  Workgroups past the table's walk the `gaps`: the elements of the
// flat store that no row covers (the stem weight, padding, a tail).  Every element is updated exactly once.
// Bits: p and buf are sgd_kernel's, wp / wpt are pack_multi_kernel's of the stored p.  hipcc contracts sgd_kernel's vector loop into three FMAs and
// its n % 4 tail into mul, add, mul, add, FMA; both forms are written out here, chosen by the element's index, so that no second contraction
// decision is involved.
__device__ __forceinline__ void sgd_update(float& p, float g, float& b, float lr, float mu, float wd) {
    const float gg = __builtin_fmaf(wd, p, g);
    b = __builtin_fmaf(mu, b, gg);
    p = __builtin_fmaf(-lr, b, p);
}
__device__ __forceinline__ void sgd_update_tail(float& p, float g, float& b, float lr, float mu, float wd) {
    const float gg = __fadd_rn(g, __fmul_rn(wd, p));
    b = __fadd_rn(__fmul_rn(mu, b), gg);
    p = __builtin_fmaf(-lr, b, p);
}

struct SgdPackArgs {
    float* p;
    const float* g;
    float* buf;
    size_t n;
    const float* sflat;
    __bf16* wp;
    __bf16* wpt;
    const long* table;         // [n_desc][8]: mi_pack_weights_multi's
    const long* gaps;          // [n_gaps][2]: [lo, hi) element ranges outside every row
    int n_desc, pack_blocks, n_gaps;
    float lr, mu, wd;
    const float* hyper;        // DEV: (lr, mu, wd) in device memory
};

constexpr int SP_TILES = 4;    // = PACK_TILES of pack_aspp.hip (the table's first_block column counts groups of that many tiles)
constexpr int SP_BATCH = 3;    // 16-byte items of p, g and buf a thread has in flight

template <bool DEV>
__global__ __launch_bounds__(256) void sgd_pack_kernel(SgdPackArgs a) {
    __shared__ float tile[32][32 * 9 + 1];
    __shared__ float ssc[32];
    const float lr = DEV ? a.hyper[0] : a.lr, mu = DEV ? a.hyper[1] : a.mu, wd = DEV ? a.hyper[2] : a.wd;
    const int tid = threadIdx.x;
    const size_t n_vec = a.n & ~(size_t)3;               // below: sgd_kernel's vector loop; from here on: its tail
    if ((int)blockIdx.x >= a.pack_blocks) {
        const long first = ((long)blockIdx.x - a.pack_blocks) * 256 + tid, stride = ((long)gridDim.x - a.pack_blocks) * 256;
        for (int k = 0; k < a.n_gaps; ++k) {
            const long lo = a.gaps[2 * k], hi = a.gaps[2 * k + 1];
            for (long i = lo + first; i < hi; i += stride) {
                float pv = a.p[i], bv = a.buf[i];
                if ((size_t)i < n_vec) sgd_update(pv, a.g[i], bv, lr, mu, wd); else sgd_update_tail(pv, a.g[i], bv, lr, mu, wd);
                a.buf[i] = bv;
                a.p[i] = pv;
            }
        }
        return;
    }
    int lo = 0, hi = a.n_desc - 1;                       // last row whose first_block <= blockIdx.x
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.table[mid * 8 + 7] <= (long)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const long* d = a.table + lo * 8;
    const int O = (int)d[4], I = (int)d[5], T = (int)d[6];
    const int tiles_i = (I + 31) >> 5, groups_i = (tiles_i + SP_TILES - 1) / SP_TILES;
    const int local = (int)((long)blockIdx.x - d[7]);
    const int ot = local / groups_i;
    const int o0 = ot * 32, it0 = (local - ot * groups_i) * SP_TILES;
    if (o0 >= O) return;
    const int no = min(32, O - o0);
    const long plane = (long)O * I;
    const bool have_t = d[3] >= 0;
    // 16-byte accesses wherever the row geometry keeps them aligned (every tile starts at a multiple of 32 input channels); element-wise otherwise
    const bool vec_ld = ((d[0] | ((long)I * T)) & 3) == 0;
    const bool vec_wp = ((d[2] | (long)I) & 7) == 0;
    const bool vec_wpt = have_t && ((d[3] | (long)O) & 7) == 0;
    if (tid < 32) ssc[tid] = (have_t && d[1] >= 0 && tid < no) ? a.sflat[d[1] + o0 + tid] : 1.f;
    for (int it = it0; it < it0 + SP_TILES && it < tiles_i; ++it) {
        const int i0 = it * 32;
        const int ni = min(32, I - i0);
        const int rowlen = ni * T;
        if (it != it0) __syncthreads();                  // the previous tile's pack reads are done
        if (vec_ld) {
            const int r4 = rowlen >> 2, items = no * r4;
            for (int base = tid; base < items; base += 256 * SP_BATCH) {
                f32x4 pv[SP_BATCH], gv[SP_BATCH], bv[SP_BATCH];
                long idx[SP_BATCH];
                int oo[SP_BATCH], ee[SP_BATCH];
#pragma unroll
                for (int j = 0; j < SP_BATCH; ++j) {
                    const int item = base + j * 256;
                    oo[j] = item / r4;
                    ee[j] = (item - oo[j] * r4) << 2;
                    idx[j] = d[0] + ((long)(o0 + oo[j]) * I + i0) * T + ee[j];
                    if (item < items) {
                        pv[j] = *reinterpret_cast<const f32x4*>(a.p + idx[j]);
                        gv[j] = *reinterpret_cast<const f32x4*>(a.g + idx[j]);
                        bv[j] = *reinterpret_cast<const f32x4*>(a.buf + idx[j]);
                    }
                }
#pragma unroll
                for (int j = 0; j < SP_BATCH; ++j) {
                    if (base + j * 256 < items) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            float pe = pv[j][e], be = bv[j][e];
                            sgd_update(pe, gv[j][e], be, lr, mu, wd);                   // a whole group of 4 below n lies below n_vec
                            pv[j][e] = pe;
                            bv[j][e] = be;
                            tile[oo[j]][ee[j] + e] = pe;
                        }
                        *reinterpret_cast<f32x4*>(a.buf + idx[j]) = bv[j];
                        *reinterpret_cast<f32x4*>(a.p + idx[j]) = pv[j];
                    }
                }
            }
        } else {
            for (int item = tid; item < no * rowlen; item += 256) {
                const int o = item / rowlen, e = item - o * rowlen;
                const long idx = d[0] + ((long)(o0 + o) * I + i0) * T + e;
                float pv = a.p[idx], bv = a.buf[idx];
                if ((size_t)idx < n_vec) sgd_update(pv, a.g[idx], bv, lr, mu, wd); else sgd_update_tail(pv, a.g[idx], bv, lr, mu, wd);
                a.buf[idx] = bv;
                a.p[idx] = pv;
                tile[o][e] = pv;
            }
        }
        __syncthreads();
        // forward operand wp[t][o][i]: 8 consecutive i per item
        if (vec_wp) {
            const int c8n = ni >> 3, per_t = no * c8n;
            for (int item = tid; item < T * per_t; item += 256) {
                const int t = item / per_t, rem = item - t * per_t;
                const int o = rem / c8n, c = (rem - o * c8n) << 3;
                bf16x8 v;
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = (__bf16)tile[o][(c + k) * T + t];
                *reinterpret_cast<bf16x8*>(a.wp + d[2] + t * plane + (long)(o0 + o) * I + i0 + c) = v;
            }
        } else {
            for (int item = tid; item < T * no * ni; item += 256) {
                const int t = item / (no * ni), rem = item - t * (no * ni);
                const int o = rem / ni, c = rem - o * ni;
                a.wp[d[2] + t * plane + (long)(o0 + o) * I + i0 + c] = (__bf16)tile[o][c * T + t];
            }
        }
        // data-gradient operand wpt[t][i][o], the FrozenBN scale of output channel o folded in: 8 consecutive o per item
        if (vec_wpt) {
            const int o8n = no >> 3, per_t = ni * o8n;
            for (int item = tid; item < T * per_t; item += 256) {
                const int t = item / per_t, rem = item - t * per_t;
                const int i = rem / o8n, o = (rem - i * o8n) << 3;
                bf16x8 v;
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = (__bf16)__fmul_rn(tile[o + k][i * T + t], ssc[o + k]);
                *reinterpret_cast<bf16x8*>(a.wpt + d[3] + t * plane + (long)(i0 + i) * O + o0 + o) = v;
            }
        } else if (have_t) {
            for (int item = tid; item < T * ni * no; item += 256) {
                const int t = item / (ni * no), rem = item - t * (ni * no);
                const int i = rem / no, o = rem - i * no;
                a.wpt[d[3] + t * plane + (long)(i0 + i) * O + o0 + o] = (__bf16)__fmul_rn(tile[o][i * T + t], ssc[o]);
            }
        }
    }
}

__global__ void relu_mask_kernel(const bf16x8* __restrict__ x, const bf16x8* __restrict__ m, bf16x8* __restrict__ y, size_t n8) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += stride) {
        const bf16x8 xv = x[i], mv = m[i];
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = ((float)mv[e] > 0.f) ? xv[e] : (__bf16)0.f;
        y[i] = o;
    }
}

// reference core/components/layers.py:18-20 (no eps)
__global__ void bn_fold_kernel(const float* w, const float* b, const float* mean, const float* var, float* scale, float* shift, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float s = w[i] * (1.0f / sqrtf(var[i]));
    scale[i] = s;
    shift[i] = b[i] - mean[i] * s;
}


extern "C" int mi_sgd_step(float* p, const float* g, float* buf, size_t n, float lr, float momentum, float weight_decay, void* stream) {
    MI_REQUIRE(p && g && buf && n > 0, "mi_sgd_step: bad argument");
    MI_REQUIRE(mi_aligned16(p) && mi_aligned16(g) && mi_aligned16(buf), "mi_sgd_step: flat buffers must be 16-byte aligned");
    const size_t n4 = n >> 2;
    size_t blocks = (n4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(sgd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, buf, n4, n, lr, momentum, weight_decay);
    MI_CHECK_LAUNCH("mi_sgd_step");
    return MI_OK;
}

extern "C" int mi_sgd_step_dev(float* p, const float* g, float* buf, size_t n, const float* hyper, void* stream) {
    MI_REQUIRE(p && g && buf && hyper && n > 0, "mi_sgd_step_dev: bad argument");
    MI_REQUIRE(mi_aligned16(p) && mi_aligned16(g) && mi_aligned16(buf), "mi_sgd_step_dev: flat buffers must be 16-byte aligned");
    const size_t n4 = n >> 2;
    size_t blocks = (n4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(sgd_dev_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, buf, n4, n, hyper);
    MI_CHECK_LAUNCH("mi_sgd_step_dev");
    return MI_OK;
}

int sgd_pack_launch(const char* who, float* p, const float* g, float* buf, size_t n, float lr, float mu, float wd, const float* hyper, bool dev,
                    const float* sflat, void* wp, void* wpt, const int64_t* table_dev, int n_desc, int total_blocks, const int64_t* gaps_dev, int n_gaps,
                    void* stream) {
    MI_REQUIRE(p && g && buf && n > 0 && wp && table_dev && n_desc > 0 && total_blocks > 0 && (!dev || hyper), "%s: bad argument", who);
    MI_REQUIRE(n_gaps >= 0 && (n_gaps == 0 || gaps_dev), "%s: n_gaps=%d without a gap table", who, n_gaps);
    MI_REQUIRE(mi_aligned16(p) && mi_aligned16(g) && mi_aligned16(buf) && mi_aligned16(wp) && mi_aligned16(wpt), "%s: buffers must be 16-byte aligned", who);
    SgdPackArgs a;
    a.p = p, a.g = g, a.buf = buf, a.n = n;
    a.sflat = sflat, a.wp = (__bf16*)wp, a.wpt = (__bf16*)wpt;
    a.table = (const long*)table_dev, a.gaps = (const long*)gaps_dev;
    a.n_desc = n_desc, a.pack_blocks = total_blocks, a.n_gaps = n_gaps;
    a.lr = lr, a.mu = mu, a.wd = wd, a.hyper = hyper;
    const unsigned grid = (unsigned)total_blocks + (n_gaps > 0 ? 64u : 0u);          // 64 workgroups walk the gaps (a few thousand elements)
    if (dev)
        hipLaunchKernelGGL(sgd_pack_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(sgd_pack_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
    MI_CHECK_LAUNCH(who);
    return MI_OK;
}

extern "C" int mi_sgd_pack_enabled(void) { return mi_sw().sgd_pack != 0; }

extern "C" int mi_sgd_step_pack(float* p, const float* g, float* buf, size_t n, float lr, float momentum, float weight_decay, const float* sflat, void* wp,
                                void* wpt, const int64_t* table_dev, int n_desc, int total_blocks, const int64_t* gaps_dev, int n_gaps, void* stream) {
    return sgd_pack_launch("mi_sgd_step_pack", p, g, buf, n, lr, momentum, weight_decay, nullptr, false, sflat, wp, wpt, table_dev, n_desc, total_blocks,
                           gaps_dev, n_gaps, stream);
}

extern "C" int mi_sgd_step_pack_dev(float* p, const float* g, float* buf, size_t n, const float* hyper, const float* sflat, void* wp, void* wpt,
                                    const int64_t* table_dev, int n_desc, int total_blocks, const int64_t* gaps_dev, int n_gaps, void* stream) {
    return sgd_pack_launch("mi_sgd_step_pack_dev", p, g, buf, n, 0.f, 0.f, 0.f, hyper, true, sflat, wp, wpt, table_dev, n_desc, total_blocks, gaps_dev,
                           n_gaps, stream);
}

__global__ void relu_mask_bits_kernel(const bf16x8* __restrict__ x, const uint8_t* __restrict__ m, bf16x8* __restrict__ y, size_t n8) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += stride) {
        const bf16x8 xv = x[i];
        const unsigned bits = m[i];              // 8 elements <-> one byte of the little-endian uint16 words
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = ((bits >> e) & 1u) ? xv[e] : (__bf16)0.f;
        y[i] = o;
    }
}

}  // namespace

extern "C" int mi_head_mask_enabled(void) { return mi_sw().head_mask != 0; }

extern "C" int mi_relu_mask(const void* x, const void* msk, void* y, size_t n, int bits, void* stream) {
    MI_REQUIRE(x && msk && y && n > 0 && n % 8 == 0, "mi_relu_mask: bad argument (n %% 8 == 0)");
    MI_REQUIRE(mi_aligned16(x) && mi_aligned16(y) && (bits || mi_aligned16(msk)), "mi_relu_mask: alignment");
    const size_t n8 = n >> 3;
    size_t blocks = (n8 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (bits) {
        MI_REQUIRE(n % 16 == 0, "mi_relu_mask: packed mask needs n %% 16 == 0");
        hipLaunchKernelGGL(relu_mask_bits_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const bf16x8*)x,
                           (const uint8_t*)msk, (bf16x8*)y, n8);
        MI_CHECK_LAUNCH("mi_relu_mask (bits)");
        return MI_OK;
    }
    hipLaunchKernelGGL(relu_mask_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const bf16x8*)x, (const bf16x8*)msk,
                       (bf16x8*)y, n8);
    MI_CHECK_LAUNCH("mi_relu_mask");
    return MI_OK;
}

extern "C" int mi_frozen_bn_fold(const float* w, const float* b, const float* mean, const float* var, float* scale, float* shift, int n,
                                 void* stream) {
    MI_REQUIRE(w && b && mean && var && scale && shift && n > 0, "mi_frozen_bn_fold: bad argument");
    hipLaunchKernelGGL(bn_fold_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, w, b, mean, var, scale, shift, n);
    MI_CHECK_LAUNCH("mi_frozen_bn_fold");
    return MI_OK;
}
