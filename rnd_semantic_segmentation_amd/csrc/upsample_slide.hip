// The sliding-window evaluation tails (TEST.SLIDE): crop-sized windows slid over the picture with an overlap, every window evaluated as
// inference() evaluates a picture (reference core/utils/utility.py:179-191), the windows' probabilities averaged where they overlap - the
// evaluation protocol of DeepLab / PSPNet on Cityscapes.  A source covers a rectangle of the output, not the whole of it.
// The per-pixel arithmetic is slide_probs (upsample_common.h); the two kernel bodies are those of the multi-source tails (upsample_score.h) with
// another value provider: arg max, thresholds, counting and the histogram are the same device code.  All arithmetic fp32.
// mi_upsample_curves_slide (TEST.CURVES) is the kernel body of upsample_curves.h with the same providers, behind the same window checks.
#include "upsample_curves.h"

namespace {

// Is every pixel of [0, H) x [0, W) inside a window?  Coordinate compression: between two neighbouring window edges of an axis every pixel has
// the same cover, so one probe per cell of the at most 129 x 129 grid of distinct edges decides.
bool all_covered(const MiSlideWindow* win, int n, int wh, int ww, int H, int W) {
    int ys[2 * MAX_SLIDE_WIN + 2], xs[2 * MAX_SLIDE_WIN + 2];
    int ny = 0, nx = 0;
    auto put = [](int* a, int& m, int v) {
        int i = 0;
        while (i < m && a[i] < v) ++i;
        if (i < m && a[i] == v) return;
        for (int j = m; j > i; --j) a[j] = a[j - 1];
        a[i] = v;
        ++m;
    };
    put(ys, ny, 0);
    put(ys, ny, H);
    put(xs, nx, 0);
    put(xs, nx, W);
    for (int i = 0; i < n; ++i) {
        put(ys, ny, win[i].y0);
        put(ys, ny, win[i].y0 + wh);
        put(xs, nx, win[i].x0);
        put(xs, nx, win[i].x0 + ww);
    }
    for (int a = 0; a + 1 < ny; ++a) {
        for (int b = 0; b + 1 < nx; ++b) {
            const int y = ys[a], x = xs[b];
            bool in = false;
            for (int i = 0; i < n && !in; ++i) in = y >= win[i].y0 && y < win[i].y0 + wh && x >= win[i].x0 && x < win[i].x0 + ww;
            if (!in) return false;
        }
    }
    return true;
}

// The windows' checks, in one order for both entries, and the descriptors for the kernel arguments.  mirror: do the windows carry mirror maps?
int slide_windows(const char* who, const MiSlideWindow* win, int n, int h, int w, int wh, int ww, int K, int H, int W, SlideWins& out, bool& mirror) {
    MI_REQUIRE(n >= 1 && n <= MAX_SLIDE_WIN, "%s: 1 <= n <= %d windows", who, MAX_SLIDE_WIN);
    MI_REQUIRE(K > 0 && K <= KMAX && H > 0 && W > 0 && h > 0 && w > 0 && wh > 0 && ww > 0, "%s: bad dimension (K <= 32)", who);
    MI_REQUIRE(wh >= h && ww >= w, "%s: only upsampling (wh >= h, ww >= w) is supported", who);
    MI_REQUIRE(wh <= H && ww <= W, "%s: a %d x %d window leaves the %d x %d output", who, wh, ww, H, W);
    mirror = win[0].low_mirror != nullptr;
    for (int i = 0; i < n; ++i) {
        const MiSlideWindow& m = win[i];
        MI_REQUIRE(m.low, "%s: window %d without a low map", who, i);
        MI_REQUIRE((m.low_mirror != nullptr) == mirror, "%s: mirror maps on some windows only (window %d)", who, i);
        MI_REQUIRE(m.y0 >= 0 && m.x0 >= 0 && m.y0 <= H - wh && m.x0 <= W - ww, "%s: window %d at (%d, %d) leaves the %d x %d output", who, i, m.y0,
                   m.x0, H, W);
    }
    MI_REQUIRE(all_covered(win, n, wh, ww, H, W), "%s: an output pixel that no window covers", who);
    for (int i = 0; i < MAX_SLIDE_WIN; ++i) {
        const MiSlideWindow& m = win[i < n ? i : 0];          // unused slots repeat window 0: never read, never uninitialised
        out.w[i] = SlideWin{m.low, m.low_mirror, m.y0, m.x0};
    }
    return MI_OK;
}

}  // namespace

extern "C" int mi_upsample_softmax_slide(const MiSlideWindow* win, int n, int h, int w, int wh, int ww, float* probs, int K, int H, int W,
                                         void* stream) {
    static const char* who = "mi_upsample_softmax_slide";
    MI_REQUIRE(win && probs, "%s: null operand", who);
    SlideWins wins;
    bool mirror;
    if (const int rc = slide_windows(who, win, n, h, w, wh, ww, K, H, W, wins, mirror)) return rc;
    const Axis ay = make_axis(h, wh), ax = make_axis(w, ww);
    if (mirror)
        launch_probs_kernel(SlideProv<true>{wins, n, ay, ax}, probs, K, H, W, stream);
    else
        launch_probs_kernel(SlideProv<false>{wins, n, ay, ax}, probs, K, H, W, stream);
    MI_CHECK_LAUNCH(who);
    return MI_OK;
}

extern "C" int mi_upsample_predict_score_slide(const MiSlideWindow* win, int n, int h, int w, int wh, int ww, int K, int H, int W,
                                               const int64_t* labels, int ignore_index, float threshold, const float* class_threshold, uint8_t* pred,
                                               uint8_t* pseudo, int64_t* counts, int bins, int64_t* hist, void* stream) {
    static const char* who = "mi_upsample_predict_score_slide";
    MI_REQUIRE(win && pred, "%s: null operand", who);
    SlideWins wins;
    bool mirror;
    if (const int rc = slide_windows(who, win, n, h, w, wh, ww, K, H, W, wins, mirror)) return rc;
    const bool cw = class_threshold != nullptr || hist != nullptr || bins != 0;      // the class-wise extras: a table, a histogram, or both
    ClassThr thr = {};
    bool ok = threshold >= 0.f && threshold <= 1.f;
    if (cw) {
        if (const int rc = classwise_table(who, K, class_threshold, pseudo, bins, hist, thr, ok)) return rc;
    } else {
        thr.t[0] = threshold;
    }
    if (const int rc = score_check(who, K, H, W, labels, ignore_index, ok, counts)) return rc;
    const Axis ay = make_axis(h, wh), ax = make_axis(w, ww);
    if (mirror)
        launch_score_kernel(SlideProv<true>{wins, n, ay, ax}, K, H, W, labels, ignore_index, thr, cw, pred, pseudo, counts, hist, stream);
    else
        launch_score_kernel(SlideProv<false>{wins, n, ay, ax}, K, H, W, labels, ignore_index, thr, cw, pred, pseudo, counts, hist, stream);
    MI_CHECK_LAUNCH(who);
    return MI_OK;
}

extern "C" int mi_upsample_curves_slide(const MiSlideWindow* win, int n, int h, int w, int wh, int ww, int K, int H, int W, const int64_t* labels,
                                        int ece_bins, int64_t* pr, int64_t* cal, void* stream) {
    static const char* who = "mi_upsample_curves_slide";
    MI_REQUIRE(win, "%s: null operand", who);
    SlideWins wins;
    bool mirror;
    if (const int rc = slide_windows(who, win, n, h, w, wh, ww, K, H, W, wins, mirror)) return rc;
    if (const int rc = curves_check(who, H, W, labels, ece_bins, pr, cal)) return rc;
    const Axis ay = make_axis(h, wh), ax = make_axis(w, ww);
    if (mirror)
        launch_curves_kernel(SlideProv<true>{wins, n, ay, ax}, K, H, W, labels, ece_bins, pr, cal, stream);
    else
        launch_curves_kernel(SlideProv<false>{wins, n, ay, ax}, K, H, W, labels, ece_bins, pr, cal, stream);
    MI_CHECK_LAUNCH(who);
    return MI_OK;
}
