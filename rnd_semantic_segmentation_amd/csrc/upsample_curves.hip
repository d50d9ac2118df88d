// Precision-recall and calibration histograms of the multi-source evaluation tail (TEST.CURVES): mi_upsample_curves.  The kernel body and its
// design notes are in upsample_curves.h; the sliding-window entry (mi_upsample_curves_slide) stands with the window checks in upsample_slide.hip.
// The per-pixel values are those of mi_upsample_softmax_multi / mi_upsample_predict_score (multi_probs through MultiProv): the histograms are
// functions of exactly the bits the probability entry writes.
#include "upsample_curves.h"

extern "C" int mi_upsample_curves(const MiProbSource* src, int n, int K, int H, int W, float div_a, float div_b, const int64_t* labels, int ece_bins,
                                  int64_t* pr, int64_t* cal, void* stream) {
    static const char* who = "mi_upsample_curves";
    MI_REQUIRE(src, "%s: null operand", who);
    MI_REQUIRE(n >= 1 && n <= MAX_PROB_SRC, "%s: 1 <= n <= 16 sources", who);
    MI_REQUIRE(K > 0 && K <= KMAX && H > 0 && W > 0, "%s: bad dimension (K <= 32)", who);
    MI_REQUIRE(div_a != 0.f && div_b != 0.f, "%s: zero divisor", who);
    if (const int rc = curves_check(who, H, W, labels, ece_bins, pr, cal)) return rc;
    ProbSrcs srcs;
    for (int i = 0; i < MAX_PROB_SRC; ++i) {
        const MiProbSource& m = src[i < n ? i : 0];       // unused slots repeat source 0: never read, never uninitialised
        MI_REQUIRE(m.low && m.h > 0 && m.w > 0, "%s: bad source", who);
        srcs.s[i] = ProbSrc{m.low, make_axis(m.h, H), make_axis(m.w, W), m.mirror != 0};
    }
    launch_curves_kernel(MultiProv{srcs, n, div_a, div_b}, K, H, W, labels, ece_bins, pr, cal, stream);
    MI_CHECK_LAUNCH(who);
    return MI_OK;
}
