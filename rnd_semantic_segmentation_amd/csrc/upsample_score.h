// The two kernel bodies of the evaluation tails, shared by the multi-source tails (upsample_infer.hip) and the sliding-window tails
// (upsample_slide.hip): the probability kernel and the predict-and-score kernel, with the per-pixel value provider as a template argument.
// A provider is a struct passed by value in the kernel arguments: the operands of its per-pixel function of upsample_common.h (multi_probs or
// slide_probs), and waves(P), the waves per SIMD the register budget is held to with P pixels per lane.  The kernels call the
// per-pixel function themselves (MI_PIXEL_VALUES below, not a member function of the provider): one more function
// level between the kernel and multi_probs made the compiler keep 202 instead of 152 VGPRs in the 19-class two-pixel scoring kernel and drop
// it from 3 waves to 2 (measured; compare the note at exp_terms in upsample_common.h).  What follows the values - arg max, thresholds,
// counting, histogram - is one piece of code for every tail.
#pragma once
#include "upsample_common.h"

namespace {

// Multi-scale, flip-averaged values (reference core/utils/utility.py:193-209): multi_probs.
// Waves per SIMD: a pixel has 4 x K corner loads in flight besides the P x K sums: one pixel per lane runs at 4 waves, two pixels per lane
// (8-byte stores, 512 contiguous bytes per wave and class plane) at 2.  Four pixels per lane spill.  No variant here does.
struct MultiProv {
    ProbSrcs srcs;
    int n;
    float div_a, div_b;
    static constexpr bool SLIDE = false;
    static constexpr int waves(int P) { return P == 1 ? 4 : 2; }
};

// Sliding-window values (upsample_slide.hip): slide_probs.  ay, ax are window-local: low map h x w -> label pixels wh x ww, the same for every
// window.  Waves per SIMD: without mirror maps a pixel holds what multi_probs holds.  With them it holds q[K] on top of the sums while the mirror
// map's 4 x K corner loads are in flight: one pixel per lane spills when held to 4 waves (36 - 104 bytes per lane) and still does in the 32-class
// instantiations when held to 3 (52 - 64 bytes), so the mirrored variants are held to 2 waves whatever the pixels per lane.  Zero scratch in every variant (the figures are in DESIGN.md 4.4g).
template <bool MIRROR_>
struct SlideProv {
    SlideWins wins;
    int n;
    Axis ay, ax;
    static constexpr bool SLIDE = true, MIRROR = MIRROR_;
    static constexpr int waves(int P) { return P == 2 || MIRROR ? 2 : 4; }
};

#define MI_PIXEL_VALUES(prov, acc)                                                                           \
    do {                                                                                                     \
        if constexpr (Prov::SLIDE)                                                                           \
            slide_probs<KR, P, Prov::MIRROR>(prov.wins.w, prov.n, K, prov.ay, prov.ax, y, xb, acc);          \
        else                                                                                                 \
            multi_probs<KR, P>(prov.srcs.s, prov.n, K, W, y, xb, prov.div_a, prov.div_b, acc);               \
    } while (0)

// probs = the provider's values.  One thread owns P consecutive pixels of a row (2 when W is even, else 1) and keeps their K values in
// registers; each class plane is written once.
template <int KT, int P, class Prov>
__global__ __launch_bounds__(256, Prov::waves(P)) void upsample_softmax_multi_kernel(Prov prov, float* __restrict__ probs, int Krt,
                                                                                                           int H, int W) {
    const int K = KT > 0 ? KT : Krt;
    constexpr int KR = KT > 0 ? KT : KMAX;
    static_assert(P == 1 || P == 2, "one or two pixels per lane");
    const int WP = W / P;                                  // P == 2 only when W is even
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)H * WP) return;
    const int xb = (int)(idx % WP) * P, y = (int)(idx / WP);
    float acc[P][KR];
    MI_PIXEL_VALUES(prov, acc);
    float* o = probs + (long)y * W + xb;
#pragma unroll
    for (int k = 0; k < KR; ++k) {
        if (k < K) {
            float* ok = o + (long)k * H * W;
            if constexpr (P == 2)
                *reinterpret_cast<float2*>(ok) = make_float2(acc[0][k], acc[1][k]);        // W even and probs 8-byte aligned (the launcher checks)
            else
                ok[0] = acc[0][k];
        }
    }
}

// Evaluation tail without the probability map: the same K values per pixel as upsample_softmax_multi_kernel, reduced in registers to
// pred = the LOWEST class index among their maxima (torch.max(dim) / numpy.argmax), pseudo = max >= threshold ? pred : 255, and - with labels -
// the integers host/metrics.py derives from pred.  One LDS add per pixel: cell gt * K + pd where the label gt lies in [0, K) (confusion_matrix;
// 255 and ignore_index lie outside [0, K)), cell K * K + pd where it does not and is not ignore_index.  From these, per class k:
//   area_intersection = cmt[k][k], area_target = row sum k, area_output = column sum k + the extra cell k.
// A workgroup sees at most 512 pixels, so its 32-bit LDS counters cannot overflow; it flushes one 64-bit global add per non-zero cell.  Integer sums
// do not depend on arrival order: the counts are bit-reproducible.  counts: [K*K] cmt, [K] intersection, [K] output, [K] target; added to.
//
// CW (mi_upsample_predict_score_cw) compiles in the two class-wise extras; without it they are gone and thr.t[0] is the one threshold:
//   - the threshold of the WINNING class: thr.t[k] travels with the running maximum through the unrolled arg-max loop, so the table is read with
//     compile-time indices (scalar registers straight from the kernel arguments), never with a per-lane index;
//   - hist[pred * 1024 + bin] += 1, bin = min(1023, int(best * 1024)): the confidence histogram per predicted class (lds_hist_add below).
constexpr int HIST_BINS = 1024;   // confidence bins per class: the cell of a pixel is pred * HIST_BINS + bin
constexpr int HIST_LINE = 16;     // cells per line of the workgroup's table: 16 neighbouring bins of one class = 128 contiguous bytes of hist
constexpr int HIST_LINES = 128;   // lines of the table (open-addressed by line number)
constexpr int HIST_PROBES = 8;    // slots tried before a pixel goes to memory directly
constexpr int HIST_PEEL = 2;      // in-wave aggregation rounds before the LDS adds
constexpr unsigned HIST_EMPTY = 0xffffffffu;

// One pixel's cell into the workgroup's table.  A dense K x 1024 table does not fit the occupancy (76 KB at K = 19), and one atomic per pixel on
// the cell itself serialises where an image is saturated (road, sky: most of a wave in ONE cell).  So:
//   1. HIST_PEEL rounds of in-wave aggregation: the lanes that hold the key of the first lane still waiting retire, their leader carries their
//      number.  A saturated wave is one LDS add after round one; a spread wave loses two ballots.
//   2. what is left goes into a table of HIST_LINES lines of HIST_LINE counters: atomicCAS claims a line for the line number cell / 16 (linear
//      probing, at most HIST_PROBES slots), atomicAdd counts in the line's counter cell % 16.  Lines, not cells, because of the flush: measured,
//      the LDS side is free and the global adds are everything - a table keyed by cell flushes one scattered 8-byte add per occupied cell,
//      each a memory request of its own, and made the kernel 3 - 4 x slower on confidences that cluster in a few dozen cells per workgroup.
//      A line flushes as 128 contiguous bytes, and the confidences of a class cluster in neighbouring bins.
//   3. a pixel that finds no line within HIST_PROBES slots (more than ~100 distinct lines in one workgroup: noise, not a segmentation) adds to
//      hist directly.  Correct for every input; only slow where nothing could be aggregated anyway.
__device__ __forceinline__ void lds_hist_add(unsigned* hline, unsigned* hcnt, unsigned long long* __restrict__ hist, unsigned key, int lane) {
    unsigned add = 1u;
    bool waiting = true;
#pragma unroll
    for (int r = 0; r < HIST_PEEL; ++r) {
        if (waiting) {
            const unsigned k0 = (unsigned)__builtin_amdgcn_readfirstlane((int)key);
            const bool same = key == k0;
            const unsigned long long m = __ballot(same);   // among the lanes still waiting
            if (same) {
                waiting = false;
                add = lane == __ffsll((long long)m) - 1 ? (unsigned)__popcll(m) : 0u;
            }
        }
    }
    if (add) {
        const unsigned line = key / HIST_LINE;
        unsigned s = (line * 2654435761u) >> 25;           // top 7 bits of the product: HIST_LINES == 1 << 7
        bool placed = false;
#pragma unroll 1
        for (int probe = 0; probe < HIST_PROBES; ++probe) {
            const unsigned prev = atomicCAS(&hline[s], HIST_EMPTY, line);
            if (prev == HIST_EMPTY || prev == line) {
                atomicAdd(&hcnt[s * HIST_LINE + key % HIST_LINE], add);
                placed = true;
                break;
            }
            s = (s + 1) & (HIST_LINES - 1);
        }
        if (!placed) atomicAdd(&hist[key], (unsigned long long)add);
    }
}

template <int KT, int P, bool CW, class Prov>
__global__ __launch_bounds__(256, Prov::waves(P)) void upsample_predict_score_kernel(Prov prov, int Krt, int H, int W,
                                                                     const long long* __restrict__ labels, int ignore_index, ClassThr thr,
                                                                     uint8_t* __restrict__ pred, uint8_t* __restrict__ pseudo,
                                                                     unsigned long long* __restrict__ counts, unsigned long long* __restrict__ hist) {
    const int K = KT > 0 ? KT : Krt;
    constexpr int KR = KT > 0 ? KT : KMAX;
    static_assert(P == 1 || P == 2, "one or two pixels per lane");
    static_assert(HIST_LINES == 128 && HIST_BINS % HIST_LINE == 0, "the hash takes 7 bits; a line never straddles two classes");
    __shared__ unsigned tab[KR * KR + KR];
    __shared__ unsigned hline[CW ? HIST_LINES : 1], hcnt[CW ? HIST_LINES * HIST_LINE : 1];
    const int tid = threadIdx.x;
    const bool with_hist = CW && hist != nullptr;          // uniform over the grid, as counts is
    if (counts) {
        for (int c = tid; c < K * K + K; c += 256) tab[c] = 0u;
    }
    if constexpr (CW) {
        if (with_hist) {
            if (tid < HIST_LINES) hline[tid] = HIST_EMPTY;
            for (int c = tid; c < HIST_LINES * HIST_LINE; c += 256) hcnt[c] = 0u;
        }
    }
    if (counts || with_hist) __syncthreads();
    const int WP = W / P;                                  // P == 2 only when W is even
    const long idx = (long)blockIdx.x * 256 + tid;
    if (idx < (long)H * WP) {
        const int xb = (int)(idx % WP) * P, y = (int)(idx / WP);
        float acc[P][KR];
        MI_PIXEL_VALUES(prov, acc);
        uint8_t pd[P], ps[P];
        float bs[P];
#pragma unroll
        for (int p = 0; p < P; ++p) {
            float best, tb;
            const int arg = first_max<CW>(acc[p], K, thr, best, tb);
            pd[p] = (uint8_t)arg;
            ps[p] = best >= tb ? (uint8_t)arg : (uint8_t)255;
            bs[p] = best;
        }
        const long o = (long)y * W + xb;
        if constexpr (P == 2) {                            // W even: o even; pred / pseudo 2-byte, labels 16-byte aligned (the launcher checks)
            *reinterpret_cast<uchar2*>(pred + o) = make_uchar2(pd[0], pd[1]);
            if (pseudo) *reinterpret_cast<uchar2*>(pseudo + o) = make_uchar2(ps[0], ps[1]);
        } else {
            pred[o] = pd[0];
            if (pseudo) pseudo[o] = ps[0];
        }
        if (counts) {
            long long gt[P];
            if constexpr (P == 2) {
                const longlong2 g = *reinterpret_cast<const longlong2*>(labels + o);
                gt[0] = g.x;
                gt[1] = g.y;
            } else {
                gt[0] = labels[o];
            }
#pragma unroll
            for (int p = 0; p < P; ++p) {
                if ((unsigned long long)gt[p] < (unsigned long long)K)
                    atomicAdd(&tab[(int)gt[p] * K + pd[p]], 1u);
                else if (gt[p] != (long long)ignore_index)
                    atomicAdd(&tab[K * K + pd[p]], 1u);
            }
        }
        if constexpr (CW) {
            if (with_hist) {
#pragma unroll
                for (int p = 0; p < P; ++p) {
                    // confidence_bin (host/metrics.py): a power-of-two scale and a truncation, both exact; the lower clamp only keeps a NaN in bounds
                    const int bin = min(HIST_BINS - 1, max(0, (int)(bs[p] * (float)HIST_BINS)));
                    lds_hist_add(hline, hcnt, hist, (unsigned)pd[p] * HIST_BINS + (unsigned)bin, tid & 63);
                }
            }
        }
    }
    if (counts || with_hist) __syncthreads();
    if (counts) {
        for (int c = tid; c < K * K; c += 256) {
            const unsigned v = tab[c];
            if (v) atomicAdd(&counts[c], (unsigned long long)v);
        }
        if (tid < K) {
            unsigned row = 0u, col = 0u;
            for (int j = 0; j < K; ++j) {
                row += tab[tid * K + j];
                col += tab[j * K + tid];
            }
            const unsigned diag = tab[tid * K + tid], out = col + tab[K * K + tid];
            if (diag) atomicAdd(&counts[K * K + tid], (unsigned long long)diag);
            if (out) atomicAdd(&counts[K * K + K + tid], (unsigned long long)out);
            if (row) atomicAdd(&counts[K * K + 2 * K + tid], (unsigned long long)row);
        }
    }
    if constexpr (CW) {
        if (with_hist) {                                   // a wave flushes 64 consecutive counters = 4 lines of 128 contiguous bytes each
            for (int c = tid; c < HIST_LINES * HIST_LINE; c += 256) {
                const unsigned v = hcnt[c];                // a counted line has its number: line * 16 + c % 16 < K * HIST_BINS by construction
                if (v) atomicAdd(&hist[hline[c / HIST_LINE] * HIST_LINE + c % HIST_LINE], (unsigned long long)v);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ launches
// Two floats per lane when W is even and probs is 8-byte aligned; the 19-class and the run-time-K instantiation.
template <class Prov>
void launch_probs_kernel(const Prov& prov, float* probs, int K, int H, int W, void* stream) {
    const bool wide = W % 2 == 0 && (reinterpret_cast<uintptr_t>(probs) & 7) == 0;
    const unsigned nb = nblk((long)H * (wide ? W / 2 : W), 256);
    with_kt(K, [&](auto kt) {
        constexpr int KT = decltype(kt)::value;
        if (wide)
            hipLaunchKernelGGL((upsample_softmax_multi_kernel<KT, 2, Prov>), dim3(nb), dim3(256), 0, (hipStream_t)stream, prov, probs, K, H, W);
        else
            hipLaunchKernelGGL((upsample_softmax_multi_kernel<KT, 1, Prov>), dim3(nb), dim3(256), 0, (hipStream_t)stream, prov, probs, K, H, W);
    });
}

// What every predict-and-score entry requires besides its sources, in the order mi_upsample_predict_score has always checked it (thr_ok is the
// caller's verdict on its threshold(s)).
inline int score_check(const char* who, int K, int H, int W, const int64_t* labels, int ignore_index, bool thr_ok, const int64_t* counts) {
    MI_REQUIRE((labels != nullptr) == (counts != nullptr), "%s: labels and counts go together", who);
    MI_REQUIRE(ignore_index < 0 || ignore_index >= K, "%s: ignore_index inside [0, K)", who);
    MI_REQUIRE(thr_ok, "%s: threshold outside [0, 1]", who);
    return MI_OK;
}

// Two pixels per lane when W is even and the byte / label pointers allow the vector accesses; with or without the class-wise extras.
template <class Prov>
void launch_score_kernel(const Prov& prov, int K, int H, int W, const int64_t* labels, int ignore_index, const ClassThr& thr, bool cw, uint8_t* pred,
                         uint8_t* pseudo, int64_t* counts, int64_t* hist, void* stream) {
    const bool wide = W % 2 == 0 && (reinterpret_cast<uintptr_t>(pred) & 1) == 0 && (reinterpret_cast<uintptr_t>(pseudo) & 1) == 0 &&
                      (reinterpret_cast<uintptr_t>(labels) & 15) == 0;
    const unsigned nb = nblk((long)H * (wide ? W / 2 : W), 256);
#define MI_LAUNCH_SCORE(KT, P, CW)                                                                                                          \
    hipLaunchKernelGGL((upsample_predict_score_kernel<KT, P, CW, Prov>), dim3(nb), dim3(256), 0, (hipStream_t)stream, prov, K, H, W,         \
                       reinterpret_cast<const long long*>(labels), ignore_index, thr, pred, pseudo, reinterpret_cast<unsigned long long*>(counts), \
                       reinterpret_cast<unsigned long long*>(hist))
#define MI_LAUNCH_SCORE_P(KT, CW) \
    do {                          \
        if (wide) MI_LAUNCH_SCORE(KT, 2, CW); else MI_LAUNCH_SCORE(KT, 1, CW); \
    } while (0)
    if (K == 19) {
        if (cw) MI_LAUNCH_SCORE_P(19, true); else MI_LAUNCH_SCORE_P(19, false);
    } else {
        if (cw) MI_LAUNCH_SCORE_P(0, true); else MI_LAUNCH_SCORE_P(0, false);
    }
#undef MI_LAUNCH_SCORE_P
#undef MI_LAUNCH_SCORE
}

// The class-wise entries' own checks and their threshold table (the checks of mi_upsample_predict_score_cw in their order).
inline int classwise_table(const char* who, int K, const float* class_threshold, const uint8_t* pseudo, int bins, const int64_t* hist, ClassThr& thr,
                           bool& ok) {
    MI_REQUIRE(!(hist && bins == 0), "%s: hist without bins", who);
    MI_REQUIRE(bins == HIST_BINS || (bins == 0 && !hist), "%s: bins must be 1024", who);
    MI_REQUIRE(class_threshold || !pseudo, "%s: pseudo without class_threshold", who);
    thr = ClassThr{};
    ok = true;
    if (class_threshold && K > 0 && K <= KMAX) {
        for (int k = 0; k < K; ++k) {
            thr.t[k] = class_threshold[k];
            ok = ok && thr.t[k] >= 0.f && thr.t[k] <= 1.f;    // false for a NaN
        }
    }
    return MI_OK;
}

}  // namespace
