"""Sliding-window evaluation of one picture (TEST.SLIDE), as ASPPTester.test() runs it, with the fused tail against the literal composition
(TEST.FUSED_SCORE False): one 1024x2048 picture, R101 + ASPP with formula weights on one MI355X, crop 769, stride 513 (2 x 4 windows), labels
1024x2048 and 2048x4096 (r = 2), with and without TEST.FLIP.

  fused    metrics.predict_and_score(slide=...) on the engine: the windows' backbone + head passes, then ONE mi_upsample_predict_score_slide
  literal  metrics.slide_inference (one mi_upsample_softmax per window - two with flip -, paste, add, count, divide: the [1,K,H,W] fp32 map),
           then the tester's statements: output.max(1), confusion_matrix, intersectionAndUnionGPU

Both paths ALTERNATE in one process after a warm-up of every shape; the clock is read after a device synchronise.  Per label size and path:
  eval     the whole evaluation of the picture (backbone included), metrics on the host
  tail     everything after the windows' 1/8-resolution logits (computed once, outside the clock)
  peak     torch.cuda.max_memory_allocated over one evaluation, above what was allocated before it
  kernels  --reps back-to-back launches between two device events, alternating: mi_upsample_predict_score_slide and mi_upsample_softmax_slide,
           beside mi_upsample_predict_score on whole-picture sources (as many as a pixel's mean cover rounded up, and the six sources of
           profiles/score_bench.txt), each also as picoseconds per evaluated softmax (one window or source on one output pixel)

    python tools/slide_bench.py [--iters 8] [--reps 20] [--precision fp32|bf16]
"""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rnd_semantic_segmentation_amd import kernels  # noqa: E402
from rnd_semantic_segmentation_amd.host import metrics, modules, synth  # noqa: E402
from score_bench import event_ms, literal_score, peak_of, timed  # noqa: E402

NUM_CLASSES = 19
SLIDE = ((769, 769), (513, 513))
PICTURE = (1024, 2048)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--precision", default="fp32", choices=("fp32", "bf16"))
    args = ap.parse_args()
    fe = modules.resnet_feature_extractor("resnet101", freeze_bn=True, pretrained_backbone=False)
    cls = modules.ASPP_Classifier_V2(2048, [6, 12, 18, 24], [6, 12, 18, 24], NUM_CLASSES)
    synth.load_formula_weights(fe)
    synth.load_formula_weights(cls)
    fe, cls = fe.cuda().eval().set_precision(args.precision), cls.cuda().eval().set_precision(args.precision)
    x = torch.from_numpy(synth.synth_image(1, PICTURE[0], PICTURE[1], seed=3)).cuda()
    with torch.no_grad():
        whole, _ = cls._lows_multi([fe(x)], [(False,)], "slide_bench")           # a whole-picture source for the multi-source yardstick
    for r in (1, 2):
        H, W = PICTURE[0] * r, PICTURE[1] * r
        y = torch.from_numpy(synth.synth_label(1, H, W, NUM_CLASSES, seed=3)).cuda().long()
        origins, (wh, ww), _ = metrics.slide_windows(PICTURE, (H, W), *SLIDE)
        lab_origins, window = [(r * a, r * b) for a, b in origins], (r * wh, r * ww)
        for flip in (False, True):
            with torch.no_grad():
                lows, mirror_lows = cls.slide_lows(metrics._slide_feats(fe, x, origins, (wh, ww), flip), flip)
            softmaxes = len(origins) * window[0] * window[1] * (2 if flip else 1)
            n_multi = int(math.ceil(softmaxes / (H * W)))

            def k_score():
                return kernels.upsample_predict_score_slide(lows, mirror_lows, lab_origins, window, (H, W), labels=y[0])

            def k_probs():
                return kernels.upsample_softmax_slide(lows, mirror_lows, lab_origins, window, (H, W))

            def k_multi(n=n_multi):
                return kernels.upsample_predict_score(whole * n, [False] * n, (H, W), float(n), 1.0, labels=y[0])

            def k_six():
                return k_multi(6)

            def fused_eval():
                res = metrics.predict_and_score(fe, cls, x, y, flip=flip, num_classes=NUM_CLASSES, slide=SLIDE)
                return res.cmt, [t.numpy() for t in (res.intersection, res.union, res.target, res.output)]

            def literal_eval():
                return literal_score(metrics.slide_inference(fe, cls, x, y, SLIDE[0], SLIDE[1], flip=flip), y)

            def fused_tail():
                return metrics.scores_from_counts(k_score()[2], NUM_CLASSES, None, None)

            def literal_tail():
                canvas = torch.zeros((1, NUM_CLASSES, H, W), dtype=torch.float32, device="cuda")
                count = torch.zeros((1, 1, H, W), dtype=torch.float32, device="cuda")
                for i, (y0, x0) in enumerate(lab_origins):
                    q = kernels.upsample_softmax(lows[i].unsqueeze(0), window, want_pred=False)[0]
                    if flip:
                        pm = kernels.upsample_softmax(mirror_lows[i].unsqueeze(0), window, want_pred=False)[0]
                        q = ((q[0] + pm[0].flip(2)) / 2).unsqueeze(0)
                    canvas[:, :, y0:y0 + window[0], x0:x0 + window[1]] += q
                    count[:, :, y0:y0 + window[0], x0:x0 + window[1]] += 1
                return literal_score(canvas / count, y)

            pairs = {"eval": (fused_eval, literal_eval), "tail": (fused_tail, literal_tail)}
            for f, l in pairs.values():                          # warm-up of every shape of both paths
                f(), l()
            same = torch.equal(fused_eval()[0], literal_eval()[0]) and torch.equal(fused_tail().cmt, literal_tail()[0])
            print("picture %dx%d, label %dx%d, %d windows of %dx%d label pixels, %s, %s (%d alternating iterations; matrices equal: %s):"
                  % (PICTURE[0], PICTURE[1], H, W, len(origins), window[0], window[1], "flip" if flip else "no flip", args.precision, args.iters, same))
            for what, (f, l) in pairs.items():
                tf, tl = [], []
                for _ in range(args.iters):                      # alternating: drift of the clocks hits both alike
                    tf.append(timed(f)[0])
                    tl.append(timed(l)[0])
                print("  %-5s fused median %8.3f ms (min %.3f, max %.3f)   literal median %8.3f ms (min %.3f, max %.3f)   literal / fused %.2f"
                      % (what, statistics.median(tf), min(tf), max(tf), statistics.median(tl), min(tl), max(tl),
                         statistics.median(tl) / statistics.median(tf)))
            print("  peak  fused %.1f MB   literal %.1f MB (the probability map alone: %.1f MB)"
                  % (peak_of(fused_eval), peak_of(literal_eval), NUM_CLASSES * H * W * 4 / 1e6))
            fns = (("predict_score_slide", k_score, softmaxes), ("softmax_slide", k_probs, softmaxes),
                   ("predict_score, %d whole-picture source%s" % (n_multi, "s" if n_multi > 1 else ""), k_multi, n_multi * H * W),
                   ("predict_score, 6 whole-picture sources", k_six, 6 * H * W))
            times = {name: [] for name, _, _ in fns}
            for _ in range(args.iters):
                for name, f, _ in fns:
                    times[name].append(event_ms(f, args.reps))
            for name, _, work in fns:
                v = times[name]
                med = statistics.median(v)
                print("  kernel %-42s median %8.1f us per call (min %.1f, max %.1f)   %.2f M softmaxes, %.1f ps each"
                      % (name, med * 1e3, min(v) * 1e3, max(v) * 1e3, work / 1e6, med * 1e9 / work))


if __name__ == "__main__":
    main()
