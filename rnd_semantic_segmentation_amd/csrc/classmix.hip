// Online self-training (mean teacher + ClassMix, the recipe of DACS / DAFormer) on the device: which classes an image holds, the pseudo-label and
// mixing pass, and the teacher's EMA update.  All three are byte-bound, enqueue-only, free of floating-point atomics and bit-reproducible.
//   mi_label_classes   labels -> one bit per class and image
//   mi_classmix        source / target images + source labels + the teacher's low-resolution logits -> mixed images and labels, without the
//                      [B,K,H,W] probability map: the pseudo-label of a pixel is the evaluation tail's (multi_probs + first_max of upsample_common.h,
//                      one source, no mirror, divisors 1 - the device code behind mi_upsample_predict_score)
//   mi_ema_update      teacher = a * teacher + (1 - a) * student over a flat fp32 store
#include "upsample_common.h"

namespace {

__device__ __forceinline__ unsigned wave_or(unsigned v) {
    for (int m = 32; m > 0; m >>= 1) v |= (unsigned)__shfl_xor((int)v, m);
    return v;
}

// ------------------------------------------------------------------------------------------------ classes present in each image
constexpr int LC_PER_THREAD = 16;                      // labels per thread: a workgroup reads 32 KiB
constexpr int LC_CHUNK = 256 * LC_PER_THREAD;          // labels per workgroup

// One workgroup per (chunk of LC_CHUNK labels, image).  A thread ORs the bits of its labels, the wave ORs its lanes (xor butterfly), the workgroup
// its four waves through LDS, and one lane issues the workgroup's single integer atomic OR.  WIDE: two labels per 16-byte load (the launcher checks
// the alignment of every image's plane).
template <bool WIDE>
__global__ __launch_bounds__(256) void label_classes_kernel(const long long* __restrict__ labels, unsigned* __restrict__ present, long HW, int K) {
    __shared__ unsigned red[4];
    const int tid = threadIdx.x, b = blockIdx.y;
    const long long* lab = labels + (long)b * HW;
    const long base = (long)blockIdx.x * LC_CHUNK;
    unsigned bits = 0u;
    if constexpr (WIDE) {
#pragma unroll
        for (int i = 0; i < LC_PER_THREAD / 2; ++i) {
            const long e = base + 2 * ((long)i * 256 + tid);              // HW is even here: a pair never straddles the end
            if (e < HW) {
                const longlong2 v = *reinterpret_cast<const longlong2*>(lab + e);
                if ((unsigned long long)v.x < (unsigned long long)K) bits |= 1u << (int)v.x;
                if ((unsigned long long)v.y < (unsigned long long)K) bits |= 1u << (int)v.y;
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < LC_PER_THREAD; ++i) {
            const long e = base + (long)i * 256 + tid;
            if (e < HW) {
                const long long v = lab[e];
                if ((unsigned long long)v < (unsigned long long)K) bits |= 1u << (int)v;
            }
        }
    }
    bits = wave_or(bits);
    if ((tid & 63) == 0) red[tid >> 6] = bits;
    __syncthreads();
    if (tid == 0) {
        const unsigned all = red[0] | red[1] | red[2] | red[3];
        if (all) atomicOr(&present[b], all);
    }
}

// ------------------------------------------------------------------------------------------------ pseudo-labels and ClassMix in one pass
// chosen(b): the ceil(n / 2) classes of present[b] with the smallest priority[b][c], n = popcount(present[b]) (n = 0: none).  Lane c < K of the
// first wave ranks class c among the present ones (priority rows are permutations: no ties); the ballot of "rank < ceil(n / 2)" is the set.
// Every workgroup recomputes it from the 4 + K bytes: no launch of its own, nothing for the host to read.
__device__ __forceinline__ unsigned chosen_classes(const unsigned* __restrict__ present, const uint8_t* __restrict__ priority, int b, int K,
                                                   unsigned* slot) {
    if (threadIdx.x < 64) {
        const int c = threadIdx.x;
        const unsigned pres = K < 32 ? present[b] & ((1u << K) - 1u) : present[b];
        const int take = (__popc(pres) + 1) >> 1;
        bool sel = false;
        if (c < K && ((pres >> c) & 1u)) {
            const uint8_t* pr = priority + (long)b * K;
            const unsigned mine = pr[c];
            int rank = 0;
            for (int o = 0; o < K; ++o) rank += (((pres >> o) & 1u) && pr[o] < mine) ? 1 : 0;
            sel = rank < take;
        }
        const unsigned long long m = __ballot(sel);
        if (threadIdx.x == 0) *slot = (unsigned)m;
    }
    __syncthreads();
    return *slot;
}

// One thread per P consecutive pixels of a row of image blockIdx.y (P = 2 when W is even and every plane keeps the alignment: 8-byte image
// accesses, 16-byte label accesses), the grid and the register budget of upsample_predict_score_kernel.  Per pixel:
//   M       = src_lab in [0, K) and in chosen(b)
//   mix_img = M ? src_img : tgt_img (three channels; only the image that is shown is read)
//   mix_lab = M ? src_lab : pseudo,  pseudo = max_k p_k >= threshold ? the lowest arg max : ignore_index,  p = the evaluation tail's K values
// A pasted pixel does not touch the teacher's logits; a wave whose pixels are all pasted skips them altogether.
// counts[b][0] += pasted pixels, counts[b][1] += unpasted pixels whose pseudo-label was kept: 32-bit sums per thread, wave, workgroup (a workgroup
// sees at most 512 pixels), then one 64-bit integer atomic add per counter and workgroup.
template <int KT, int P>
__global__ __launch_bounds__(256, P == 1 ? 4 : 2) void classmix_kernel(const float* __restrict__ src_img, const float* __restrict__ tgt_img,
                                                                       const long long* __restrict__ src_lab, const float* __restrict__ teacher_low,
                                                                       const unsigned* __restrict__ present, const uint8_t* __restrict__ priority,
                                                                       ClassThr thr, long long ignore_index, float* __restrict__ mix_img,
                                                                       long long* __restrict__ mix_lab, uint8_t* __restrict__ mask,
                                                                       unsigned long long* __restrict__ counts, int Krt, Axis ay, Axis ax) {
    const int K = KT > 0 ? KT : Krt;
    constexpr int KR = KT > 0 ? KT : KMAX;
    static_assert(P == 1 || P == 2, "one or two pixels per lane");
    __shared__ unsigned chosen_slot, red[4][2];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int H = ay.n_out, W = ax.n_out;
    const unsigned chosen = chosen_classes(present, priority, b, K, &chosen_slot);
    const int WP = W / P;                                  // P == 2 only when W is even
    const long idx = (long)blockIdx.x * 256 + tid;
    unsigned n_paste = 0u, n_kept = 0u;
    if (idx < (long)H * WP) {
        const int xb = (int)(idx % WP) * P, y = (int)(idx / WP);
        const long plane = (long)H * W;
        const long o = (long)y * W + xb;                   // within one [H][W] plane
        const long ol = (long)b * plane + o;               // within a [B][H][W] tensor
        long long lab[P];
        if constexpr (P == 2) {
            const longlong2 g = *reinterpret_cast<const longlong2*>(src_lab + ol);
            lab[0] = g.x;
            lab[1] = g.y;
        } else {
            lab[0] = src_lab[ol];
        }
        bool M[P];
#pragma unroll
        for (int p = 0; p < P; ++p) M[p] = (unsigned long long)lab[p] < (unsigned long long)K && ((chosen >> (int)lab[p]) & 1u);
        // images: the P pixels of a lane come from one image each; both are read only where a lane shows one pixel of each
        const long oi = (long)b * 3 * plane + o;
        if constexpr (P == 2) {
            const bool any_s = M[0] || M[1], any_t = !(M[0] && M[1]);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float2 s = make_float2(0.f, 0.f), t = make_float2(0.f, 0.f);
                if (any_s) s = *reinterpret_cast<const float2*>(src_img + oi + c * plane);
                if (any_t) t = *reinterpret_cast<const float2*>(tgt_img + oi + c * plane);
                *reinterpret_cast<float2*>(mix_img + oi + c * plane) = make_float2(M[0] ? s.x : t.x, M[1] ? s.y : t.y);
            }
        } else {
            const float* from = M[0] ? src_img : tgt_img;
#pragma unroll
            for (int c = 0; c < 3; ++c) mix_img[oi + c * plane] = from[oi + c * plane];
        }
        // labels: the source label where pasted, else the teacher's pseudo-label
        long long out[P];
        ProbSrc src;
        src.low = teacher_low + (long)b * ay.n_in * ax.n_in * K;
        src.ay = ay;
        src.ax = ax;
        src.mirror = 0;
#pragma unroll
        for (int p = 0; p < P; ++p) {
            if (M[p]) {
                out[p] = lab[p];
                ++n_paste;
            } else {
                float acc[1][KR];
                multi_probs<KR, 1>(&src, 1, K, W, y, xb + p, 1.f, 1.f, acc);
                float best, tb;
                const int arg = first_max<false>(acc[0], K, thr, best, tb);
                const bool keep = best >= tb;
                out[p] = keep ? (long long)arg : ignore_index;
                n_kept += keep ? 1u : 0u;
            }
        }
        if constexpr (P == 2) {                            // W even: o even; labels 16-byte, mask 2-byte aligned (the launcher checks)
            longlong2 g;
            g.x = out[0];
            g.y = out[1];
            *reinterpret_cast<longlong2*>(mix_lab + ol) = g;
            if (mask) *reinterpret_cast<uchar2*>(mask + ol) = make_uchar2(M[0] ? 1 : 0, M[1] ? 1 : 0);
        } else {
            mix_lab[ol] = out[0];
            if (mask) mask[ol] = M[0] ? 1 : 0;
        }
    }
    n_paste = wave_sum(n_paste);
    n_kept = wave_sum(n_kept);
    if ((tid & 63) == 0) {
        red[tid >> 6][0] = n_paste;
        red[tid >> 6][1] = n_kept;
    }
    __syncthreads();
    if (tid < 2) {
        const unsigned v = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
        if (v) atomicAdd(&counts[(long)b * 2 + tid], (unsigned long long)v);
    }
}

// ------------------------------------------------------------------------------------------------ the teacher's EMA update
typedef float f32x4_any __attribute__((ext_vector_type(4), aligned(4)));      // a 16-byte access at any 4-byte alignment

__device__ __forceinline__ float ema_mix(float a, float t, float b, float s) {
#pragma clang fp contract(off)
    const float at = a * t, bs = b * s;
    return at + bs;
}

// teacher[i] = a * teacher[i] + b * student[i] with a = hyper[0] read from device memory (a captured HIP graph replays with whatever the host
// wrote there) and b the fp32 difference 1 - a; both products and the sum rounded (ema_mix: contraction off), the same for every element.
// The stores hand out the ranges: `head` elements bring the teacher pointer to a 16-byte boundary (scalar), then n4 aligned 16-byte groups - the
// student side of a group is a 16-byte load at whatever 4-byte alignment it has - then the n - head - 4 n4 < 4 elements that are left (scalar).
__global__ __launch_bounds__(256) void ema_kernel(float* __restrict__ teacher, const float* __restrict__ student, size_t head, size_t n4, size_t n,
                                                  const float* __restrict__ hyper) {
    const float a = hyper[0], b = 1.0f - a;
    f32x4* t4 = reinterpret_cast<f32x4*>(teacher + head);
    const f32x4_any* s4 = reinterpret_cast<const f32x4_any*>(student + head);
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        f32x4 tv = t4[i];
        const f32x4_any sv = s4[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) tv[e] = ema_mix(a, tv[e], b, sv[e]);
        t4[i] = tv;
    }
    if (blockIdx.x == 0 && threadIdx.x < 8) {              // lanes 0..3: the head, lanes 4..7: the tail
        const size_t tail0 = head + (n4 << 2);
        const size_t i = threadIdx.x < 4 ? (size_t)threadIdx.x : tail0 + (threadIdx.x - 4);
        const bool mine = threadIdx.x < 4 ? (size_t)threadIdx.x < head : i < n;
        if (mine) teacher[i] = ema_mix(a, teacher[i], b, student[i]);
    }
}

}  // namespace

extern "C" int mi_label_classes(const int64_t* labels, uint32_t* present, int B, int H, int W, int K, void* stream) {
    MI_REQUIRE(labels && present, "mi_label_classes: null operand");
    MI_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0, "mi_label_classes: bad dimension (B = %d, H = %d, W = %d)", B, H, W);
    MI_REQUIRE(K >= 1 && K <= KMAX, "mi_label_classes: K = %d outside 1..32", K);
    const long HW = (long)H * W;
    if (hipMemsetAsync(present, 0, (size_t)B * sizeof(uint32_t), (hipStream_t)stream) != hipSuccess)
        return mi_set_error(MI_EHIP, "mi_label_classes: memset failed");
    const dim3 grid(nblk(HW, LC_CHUNK), B);
    const bool wide = HW % 2 == 0 && mi_aligned16(labels);
    if (wide)
        hipLaunchKernelGGL(label_classes_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const long long*>(labels), present, HW, K);
    else
        hipLaunchKernelGGL(label_classes_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const long long*>(labels), present, HW, K);
    MI_CHECK_LAUNCH("mi_label_classes");
    return MI_OK;
}

extern "C" int mi_classmix(const float* src_img, const float* tgt_img, const int64_t* src_lab, const float* teacher_low, const uint32_t* present,
                           const uint8_t* priority, float threshold, int ignore_index, float* mix_img, int64_t* mix_lab, uint8_t* mask,
                           int64_t* counts, int B, int h, int w, int K, int H, int W, void* stream) {
    MI_REQUIRE(src_img && tgt_img && src_lab && teacher_low && present && priority && mix_img && mix_lab && counts, "mi_classmix: null operand");
    MI_REQUIRE(B > 0 && B <= 65535 && h > 0 && w > 0 && H > 0 && W > 0, "mi_classmix: bad dimension (B = %d, h = %d, w = %d, H = %d, W = %d)", B, h, w, H, W);
    MI_REQUIRE(H >= h && W >= w, "mi_classmix: the teacher's logits are upsampled (H = %d < h = %d or W = %d < w = %d)", H, h, W, w);
    MI_REQUIRE(K >= 1 && K <= KMAX, "mi_classmix: K = %d outside 1..32", K);
    MI_REQUIRE(threshold >= 0.f && threshold <= 1.f, "mi_classmix: threshold outside [0, 1]");      // false for a NaN
    MI_REQUIRE(ignore_index < 0 || ignore_index >= K, "mi_classmix: ignore_index inside [0, K)");
    if (hipMemsetAsync(counts, 0, (size_t)B * 2 * sizeof(int64_t), (hipStream_t)stream) != hipSuccess)
        return mi_set_error(MI_EHIP, "mi_classmix: memset failed");
    ClassThr thr = {};
    thr.t[0] = threshold;
    const auto a8 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; };
    const bool wide = W % 2 == 0 && a8(src_img) && a8(tgt_img) && a8(mix_img) && mi_aligned16(src_lab) && mi_aligned16(mix_lab) &&
                      (reinterpret_cast<uintptr_t>(mask) & 1) == 0;
    const dim3 grid(nblk((long)H * (wide ? W / 2 : W), 256), B);
    const Axis ay = make_axis(h, H), ax = make_axis(w, W);
#define MI_LAUNCH_MIX(KT, P)                                                                                                                       \
    hipLaunchKernelGGL((classmix_kernel<KT, P>), grid, dim3(256), 0, (hipStream_t)stream, src_img, tgt_img, reinterpret_cast<const long long*>(src_lab), \
                       teacher_low, present, priority, thr, (long long)ignore_index, mix_img, reinterpret_cast<long long*>(mix_lab), mask,         \
                       reinterpret_cast<unsigned long long*>(counts), K, ay, ax)
    if (K == 19) {
        if (wide) MI_LAUNCH_MIX(19, 2); else MI_LAUNCH_MIX(19, 1);
    } else {
        if (wide) MI_LAUNCH_MIX(0, 2); else MI_LAUNCH_MIX(0, 1);
    }
#undef MI_LAUNCH_MIX
    MI_CHECK_LAUNCH("mi_classmix");
    return MI_OK;
}

extern "C" int mi_ema_update(float* teacher, const float* student, size_t n, const float* hyper, void* stream) {
    MI_REQUIRE(teacher && student && hyper, "mi_ema_update: null operand");
    MI_REQUIRE(n > 0, "mi_ema_update: n = 0");
    MI_REQUIRE((reinterpret_cast<uintptr_t>(teacher) & 3) == 0 && (reinterpret_cast<uintptr_t>(student) & 3) == 0 &&
                   (reinterpret_cast<uintptr_t>(hyper) & 3) == 0, "mi_ema_update: pointers must be 4-byte aligned");
    size_t head = ((16 - (reinterpret_cast<uintptr_t>(teacher) & 15)) & 15) / 4;      // floats up to the teacher's next 16-byte boundary
    if (head > n) head = n;
    const size_t n4 = (n - head) / 4;
    unsigned nb = nblk((long)(n4 ? n4 : 1), 256);
    if (nb > 2048) nb = 2048;                              // grid-stride above 8 workgroups per CU
    hipLaunchKernelGGL(ema_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, teacher, student, head, n4, n, hyper);
    MI_CHECK_LAUNCH("mi_ema_update");
    return MI_OK;
}
