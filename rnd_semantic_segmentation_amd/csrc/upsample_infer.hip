// The inference tails on bilinearly upsampled logits: softmax probabilities (one source, or multi-scale and flip-averaged), the evaluation tail
// that reduces them to predictions, pseudo-labels and score counts, and the align_corners image resize.
//   softmax over classes for inference                        reference core/utils/utility.py:186
// All arithmetic fp32.  They share only the source-index arithmetic (Axis) and the exponential loop with the training heads of upsample_ce.hip.
#include "upsample_score.h"

namespace {

// ------------------------------------------------------------------------------------------------ inference tails
// The per-source arithmetic of both inference tails (interp_softmax_terms) and the per-pixel arithmetic of the multi-scale tails (multi_probs, first_max)
// live in upsample_common.h: the ClassMix pass of classmix.hip draws its pseudo-labels from the same device code.  The multi-source probability
// kernel and the predict-and-score kernel live in upsample_score.h, where the sliding-window tails (upsample_slide.hip) share their bodies.
// probs NCHW + optional argmax
__global__ void upsample_softmax_kernel(const float* __restrict__ low, float* __restrict__ probs, uint8_t* __restrict__ pred, int B, int K,
                                        Axis ay, Axis ax) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int H = ay.n_out, W = ax.n_out, h = ay.n_in, w = ax.n_in;
    if (idx >= (long)B * H * W) return;
    const int x = (int)(idx % W), y = (int)((idx / W) % H), b = (int)(idx / ((long)W * H));
    float v[KMAX];
    int arg;
    const float rse = interp_softmax_terms<KMAX>(low + (long)b * h * w * K, K, ay, ax, y, x, v, arg);
    float* o = probs + ((long)b * K * H + y) * W + x;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        if (k < K) o[(long)k * H * W] = v[k] * rse;
    }
    if (pred) pred[idx] = (uint8_t)arg;
}


// F.interpolate(x, (Ho, Wo), mode='bilinear', align_corners=True) on NCHW fp32 images; with_mirror: image b's horizontal mirror
// (torch.flip(resized, [3])) is written as image B + b from the same registers, so the two halves are bit-equal mirrors.
__global__ void image_resize_ac_kernel(const float* __restrict__ x, float* __restrict__ out, int B, int C, Axis ay, Axis ax, int with_mirror) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int Ho = ay.n_out, Wo = ax.n_out, H = ay.n_in, W = ax.n_in;
    if (idx >= (long)B * C * Ho * Wo) return;
    const int xo = (int)(idx % Wo), yo = (int)((idx / Wo) % Ho);
    const long bc = idx / ((long)Wo * Ho);
    int y0, y1, x0, x1;
    float ly, lx;
    ay.src(yo, y0, y1, ly);
    ax.src(xo, x0, x1, lx);
    const float* p = x + bc * H * W;
    const float v00 = p[(long)y0 * W + x0];
    // on a grid point (every pixel when the size does not change) the value is the input's, bit for bit (-0 and non-finite neighbours included)
    const float val = (lx == 0.f && ly == 0.f) ? v00 : lerp2(v00, p[(long)y0 * W + x1], p[(long)y1 * W + x0], p[(long)y1 * W + x1], lx, ly);
    out[idx] = val;
    if (with_mirror) out[((bc + (long)B * C) * Ho + yo) * Wo + (Wo - 1 - xo)] = val;
}

}  // namespace

extern "C" int mi_upsample_softmax(const float* low, float* probs, uint8_t* pred, int B, int h, int w, int K, int H, int W, void* stream) {
    MI_REQUIRE(low && probs && B > 0 && h > 0 && w > 0 && H > 0 && W > 0 && K > 0 && K <= KMAX, "mi_upsample_softmax: bad argument (K <= 32)");
    hipLaunchKernelGGL(upsample_softmax_kernel, dim3(nblk((long)B * H * W, 256)), dim3(256), 0, (hipStream_t)stream, low, probs, pred, B, K,
                       make_axis(h, H), make_axis(w, W));
    MI_CHECK_LAUNCH("mi_upsample_softmax");
    return MI_OK;
}

extern "C" int mi_upsample_softmax_multi(const MiProbSource* src, int n, float* probs, int K, int H, int W, float div_a, float div_b,
                                         void* stream) {
    MI_REQUIRE(src && probs, "mi_upsample_softmax_multi: null operand");
    MI_REQUIRE(n >= 1 && n <= MAX_PROB_SRC, "mi_upsample_softmax_multi: 1 <= n <= 16 sources");
    MI_REQUIRE(K > 0 && K <= KMAX && H > 0 && W > 0, "mi_upsample_softmax_multi: bad dimension (K <= 32)");
    MI_REQUIRE(div_a != 0.f && div_b != 0.f, "mi_upsample_softmax_multi: zero divisor");
    ProbSrcs srcs;
    for (int i = 0; i < MAX_PROB_SRC; ++i) {
        const MiProbSource& m = src[i < n ? i : 0];       // unused slots repeat source 0: never read, never uninitialised
        MI_REQUIRE(m.low && m.h > 0 && m.w > 0, "mi_upsample_softmax_multi: bad source");
        srcs.s[i] = ProbSrc{m.low, make_axis(m.h, H), make_axis(m.w, W), m.mirror != 0};
    }
    launch_probs_kernel(MultiProv{srcs, n, div_a, div_b}, probs, K, H, W, stream);
    MI_CHECK_LAUNCH("mi_upsample_softmax_multi");
    return MI_OK;
}

// The one launcher of both evaluation-tail entries: the checks of mi_upsample_predict_score in their order (thr_ok is the caller's verdict on
// its threshold(s)), then the core with or without the class-wise extras.
static int launch_predict_score(const char* who, const MiProbSource* src, int n, int K, int H, int W, float div_a, float div_b, const int64_t* labels,
                                int ignore_index, bool thr_ok, const ClassThr& thr, bool cw, uint8_t* pred, uint8_t* pseudo, int64_t* counts,
                                int64_t* hist, void* stream) {
    MI_REQUIRE(src && pred, "%s: null operand", who);
    MI_REQUIRE(n >= 1 && n <= MAX_PROB_SRC, "%s: 1 <= n <= 16 sources", who);
    MI_REQUIRE(K > 0 && K <= KMAX && H > 0 && W > 0, "%s: bad dimension (K <= 32)", who);
    MI_REQUIRE(div_a != 0.f && div_b != 0.f, "%s: zero divisor", who);
    if (const int rc = score_check(who, K, H, W, labels, ignore_index, thr_ok, counts)) return rc;
    ProbSrcs srcs;
    for (int i = 0; i < MAX_PROB_SRC; ++i) {
        const MiProbSource& m = src[i < n ? i : 0];       // unused slots repeat source 0: never read, never uninitialised
        MI_REQUIRE(m.low && m.h > 0 && m.w > 0, "%s: bad source", who);
        srcs.s[i] = ProbSrc{m.low, make_axis(m.h, H), make_axis(m.w, W), m.mirror != 0};
    }
    launch_score_kernel(MultiProv{srcs, n, div_a, div_b}, K, H, W, labels, ignore_index, thr, cw, pred, pseudo, counts, hist, stream);
    MI_CHECK_LAUNCH(who);
    return MI_OK;
}

extern "C" int mi_upsample_predict_score(const MiProbSource* src, int n, int K, int H, int W, float div_a, float div_b, const int64_t* labels,
                                         int ignore_index, float threshold, uint8_t* pred, uint8_t* pseudo, int64_t* counts, void* stream) {
    ClassThr thr = {};
    thr.t[0] = threshold;
    return launch_predict_score("mi_upsample_predict_score", src, n, K, H, W, div_a, div_b, labels, ignore_index, threshold >= 0.f && threshold <= 1.f,
                                thr, false, pred, pseudo, counts, nullptr, stream);
}

extern "C" int mi_upsample_predict_score_cw(const MiProbSource* src, int n, int K, int H, int W, float div_a, float div_b, const int64_t* labels,
                                            int ignore_index, const float* class_threshold, uint8_t* pred, uint8_t* pseudo, int64_t* counts,
                                            int bins, int64_t* hist, void* stream) {
    static const char* who = "mi_upsample_predict_score_cw";
    ClassThr thr;
    bool ok;
    if (const int rc = classwise_table(who, K, class_threshold, pseudo, bins, hist, thr, ok)) return rc;
    return launch_predict_score(who, src, n, K, H, W, div_a, div_b, labels, ignore_index, ok, thr, true, pred, pseudo, counts, hist, stream);
}

extern "C" int mi_image_resize_ac(const float* x, float* out, int B, int C, int H, int W, int Ho, int Wo, int with_mirror, void* stream) {
    MI_REQUIRE(x && out && B > 0 && C > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0, "mi_image_resize_ac: bad argument");
    hipLaunchKernelGGL(image_resize_ac_kernel, dim3(nblk((long)B * C * Ho * Wo, 256)), dim3(256), 0, (hipStream_t)stream, x, out, B, C,
                       make_axis(H, Ho), make_axis(W, Wo), with_mirror != 0);
    MI_CHECK_LAUNCH("mi_image_resize_ac");
    return MI_OK;
}
