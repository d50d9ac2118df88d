// The kernel body of the curve tails (TEST.CURVES; mi_upsample_curves in upsample_curves.hip, mi_upsample_curves_slide in upsample_slide.hip):
// per-class precision-recall histograms and the calibration histogram of one picture, from the per-pixel values of the evaluation tails
// (the providers and MI_PIXEL_VALUES of upsample_score.h, untouched) and the label.  The definition: include/mi355seg.h.  Per counted pixel
// (label in [0, K)) the kernel makes K adds into pr[k][bin(p_k)][label == k] and one into cal[bin(max)]: integers only, no floating-point
// atomics, so the sums do not depend on arrival order and two calls give the same bits.
//   table     dense, in dynamic LDS: [M][3] 64-bit calibration cells, then [K][256][2] 32-bit counters in the layout of pr.  2048 K + 24 M bytes:
//             39 272 at K = 19, M = 15 (4 workgroups per CU by LDS; 2 - 4 by registers, per instantiation in DESIGN.md 4.4i), 67 072 at K = 32,
//             M = 64 (2 per CU; above the static limit, hence dynamic).  A hashed table as in lds_hist_add does not fit K adds per pixel into up to 512 K cells.
//   adds      on a trained net nearly every pixel sends K - 1 adds to (k, 0, negative) and one to (arg max, 255, positive), and an LDS atomic
//             per lane would serialise the wave on one address.  Per class and pixel slot two ballots pick those two cells out; lanes 0 and 1
//             add the popcounts.  Only what is left takes an LDS atomic of its own.
//   cal       one aggregation round on the bin of the first live lane (ballots for the count and the hits, a wave sum for the fixed-point
//             confidences: 64 x (2^24 + 1) < 2^32), the leader adds three 64-bit LDS cells; the other lanes add theirs one by one.
//   grid      capped at CV_MAX_GRID workgroups; a workgroup strides over the tiles of 256 P pixels and flushes ONCE, one 64-bit global add per
//             non-zero cell, in the order of pr (a wave covers 64 consecutive cells = 512 contiguous bytes).
//   overflow  the launchers refuse H * W >= 2^31, so a 32-bit LDS counter cannot overflow whatever the grid; a 64-bit calibration cell holds at
//             most 2^31 x (2^24 + 1) < 2^56 per launch.
#pragma once
#include "upsample_score.h"

namespace {

constexpr int CV_BINS = 256;          // CURVE_BINS of host/metrics.py
constexpr int CV_MAX_ECE = 64;        // ece_bins at most
constexpr long CV_MAX_GRID = 1024;    // workgroups at most: four per CU on 256 CUs.  Only the one-pixel-per-lane instantiations without mirror maps hold four
                                      // (registers; LDS allows four at K = 19, two at K = 32); the others hold two or three and run the rest as a tail
                                      // (DESIGN.md 4.4i has the table; a cap sized by the instantiation's occupancy has not been tried)

typedef unsigned long long cv_u64;

inline size_t curves_lds_bytes(int K, int M) { return (size_t)M * 3 * sizeof(cv_u64) + (size_t)K * CV_BINS * 2 * sizeof(unsigned); }

template <int KT, int P, class Prov>
__global__ __launch_bounds__(256, Prov::waves(P)) void upsample_curves_kernel(Prov prov, int Krt, int H, int W, const long long* __restrict__ labels,
                                                                              int M, long ntiles, cv_u64* __restrict__ pr, cv_u64* __restrict__ cal) {
    const int K = KT > 0 ? KT : Krt;
    constexpr int KR = KT > 0 ? KT : KMAX;
    static_assert(P == 1 || P == 2, "one or two pixels per lane");
    extern __shared__ __attribute__((aligned(16))) unsigned char cv_lds[];
    cv_u64* ctab = reinterpret_cast<cv_u64*>(cv_lds);                       // [M][3]
    unsigned* tab = reinterpret_cast<unsigned*>(cv_lds + (size_t)M * 3 * sizeof(cv_u64));      // [K][256][2]
    const int tid = threadIdx.x, lane = tid & 63;
    const int cells = K * CV_BINS * 2;
    if (pr) {
        for (int c = tid; c < cells; c += 256) tab[c] = 0u;
    }
    if (cal) {
        for (int c = tid; c < M * 3; c += 256) ctab[c] = 0ull;
    }
    __syncthreads();
    const int WP = W / P;                                  // P == 2 only when W is even
    const long npx = (long)H * WP;
    for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {      // workgroup-uniform: every lane of a wave takes every ballot below
        const long idx = t * 256 + tid;
        const bool live = idx < npx;
        const long at = live ? idx : 0;                    // a lane beyond the picture computes pixel 0 and counts nothing
        const int xb = (int)(at % WP) * P, y = (int)(at / WP);
        float acc[P][KR];
        MI_PIXEL_VALUES(prov, acc);
        const long o = (long)y * W + xb;
        long long gt[P];
        if constexpr (P == 2) {                            // W even: o even; labels 16-byte aligned (the launcher checks)
            const longlong2 g = *reinterpret_cast<const longlong2*>(labels + o);
            gt[0] = g.x;
            gt[1] = g.y;
        } else {
            gt[0] = labels[o];
        }
        bool cnt[P];
        int cls[P];
#pragma unroll
        for (int p = 0; p < P; ++p) {
            cnt[p] = live && (unsigned long long)gt[p] < (unsigned long long)K;      // the confusion matrix's rule
            cls[p] = cnt[p] ? (int)gt[p] : -1;
        }
        if (pr) {
#pragma unroll
            for (int k = 0; k < KR; ++k) {
                if (k < K) {
                    unsigned n0 = 0u, n1 = 0u;
#pragma unroll
                    for (int p = 0; p < P; ++p) {
                        // a power-of-two scale and a truncation, both exact; the lower clamp only keeps a NaN in bounds
                        const int bin = min(CV_BINS - 1, max(0, (int)(acc[p][k] * (float)CV_BINS)));
                        const bool pos = cls[p] == k;
                        const bool low = cnt[p] && bin == 0 && !pos, top = cnt[p] && bin == CV_BINS - 1 && pos;
                        n0 += (unsigned)__popcll(__ballot(low));
                        n1 += (unsigned)__popcll(__ballot(top));
                        if (cnt[p] && !low && !top) atomicAdd(&tab[(k * CV_BINS + bin) * 2 + (pos ? 1 : 0)], 1u);
                    }
                    if (lane == 0 && n0) atomicAdd(&tab[k * CV_BINS * 2], n0);
                    if (lane == 1 && n1) atomicAdd(&tab[(k * CV_BINS + CV_BINS - 1) * 2 + 1], n1);
                }
            }
        }
        if (cal) {
#pragma unroll
            for (int p = 0; p < P; ++p) {
                float best = acc[p][0];
                int arg = 0;
#pragma unroll
                for (int k = 1; k < KR; ++k) {
                    if (k < K && acc[p][k] > best) {       // strict: the first of equal maxima stays
                        best = acc[p][k];
                        arg = k;
                    }
                }
                const int m = min(M - 1, max(0, (int)(best * (float)M)));
                const unsigned fx = (unsigned)(int)(best * 16777216.f);      // 2^24: an exact scale, a truncation
                const bool hit = arg == cls[p];
                bool waiting = cnt[p];
                const cv_u64 act = __ballot(waiting);
                if (act) {                                 // wave-uniform
                    const int lead = __ffsll((long long)act) - 1;
                    const int m0 = __shfl(m, lead);
                    const bool same = waiting && m == m0;
                    const cv_u64 ms = __ballot(same), mh = __ballot(same && hit);
                    const unsigned s = wave_sum(same ? fx : 0u);
                    if (lane == lead) {
                        atomicAdd(&ctab[m0 * 3], (cv_u64)__popcll(ms));
                        if (mh) atomicAdd(&ctab[m0 * 3 + 1], (cv_u64)__popcll(mh));
                        atomicAdd(&ctab[m0 * 3 + 2], (cv_u64)s);
                    }
                    waiting = waiting && !same;
                }
                if (waiting) {
                    atomicAdd(&ctab[m * 3], 1ull);
                    if (hit) atomicAdd(&ctab[m * 3 + 1], 1ull);
                    atomicAdd(&ctab[m * 3 + 2], (cv_u64)fx);
                }
            }
        }
    }
    __syncthreads();
    if (pr) {
        for (int c = tid; c < cells; c += 256) {
            const unsigned v = tab[c];
            if (v) atomicAdd(&pr[c], (cv_u64)v);
        }
    }
    if (cal) {
        for (int c = tid; c < M * 3; c += 256) {
            const cv_u64 v = ctab[c];
            if (v) atomicAdd(&cal[c], v);
        }
    }
}

// What both curve entries require besides their sources or windows.
inline int curves_check(const char* who, int H, int W, const int64_t* labels, int ece_bins, const int64_t* pr, const int64_t* cal) {
    MI_REQUIRE(labels, "%s: null labels", who);
    MI_REQUIRE(pr || cal, "%s: neither pr nor cal", who);
    MI_REQUIRE(!cal || (ece_bins >= 1 && ece_bins <= CV_MAX_ECE), "%s: ece_bins %d lies outside 1..%d", who, ece_bins, CV_MAX_ECE);
    MI_REQUIRE((long)H * W < (1l << 31), "%s: H * W = %ld reaches 2^31", who, (long)H * W);
    return MI_OK;
}

// One launch; the table may pass 64 KB (K = 32), which has to be allowed once per (kernel, device).
template <auto Kern, class Prov>
void launch_curves_one(const Prov& prov, unsigned nb, size_t lds, hipStream_t st, int K, int H, int W, const int64_t* labels, int M, long ntiles,
                       int64_t* pr, int64_t* cal) {
    static std::atomic<uint64_t> lds_set;
    mi_allow_dynamic_lds((const void*)Kern, MI_LDS_MAX, lds_set);
    hipLaunchKernelGGL(Kern, dim3(nb), dim3(256), lds, st, prov, K, H, W, reinterpret_cast<const long long*>(labels), M, ntiles,
                       reinterpret_cast<cv_u64*>(pr), reinterpret_cast<cv_u64*>(cal));
}

// Two pixels per lane when W is even and the labels allow the 16-byte loads; the 19-class and the run-time-K instantiation; a capped grid.
template <class Prov>
void launch_curves_kernel(const Prov& prov, int K, int H, int W, const int64_t* labels, int ece_bins, int64_t* pr, int64_t* cal, void* stream) {
    const bool wide = W % 2 == 0 && (reinterpret_cast<uintptr_t>(labels) & 15) == 0;
    const long ntiles = nblk((long)H * (wide ? W / 2 : W), 256);
    const unsigned nb = (unsigned)(ntiles < CV_MAX_GRID ? ntiles : CV_MAX_GRID);
    const int M = cal ? ece_bins : 0;
    const size_t lds = curves_lds_bytes(pr ? K : 0, M);
    with_kt(K, [&](auto kt) {
        constexpr int KT = decltype(kt)::value;
        if (wide)
            launch_curves_one<upsample_curves_kernel<KT, 2, Prov>>(prov, nb, lds, (hipStream_t)stream, K, H, W, labels, M, ntiles, pr, cal);
        else
            launch_curves_one<upsample_curves_kernel<KT, 1, Prov>>(prov, nb, lds, (hipStream_t)stream, K, H, W, labels, M, ntiles, pr, cal);
    });
}

}  // namespace
