"""Evaluation of one image, as ASPPTester.test() runs it, with the fused scoring tail against the literal one (TEST.FUSED_SCORE False): one
512x1024 image, labels 512x1024 and 1024x2048, R101 + ASPP with formula weights on one MI355X, single scale and scales [0.7, 1.0, 1.3] with flip.

  fused    metrics.predict_and_score on the engine: backbone + head passes, then ONE mi_upsample_predict_score (argmax, threshold, counts), one
           device-to-host copy of the counts; --saveres copies the 1-byte mask
  literal  the tester's statements without it: inference / multi_scale_inference (the [1,K,H,W] fp32 map), output.max(1), confusion_matrix,
           intersectionAndUnionGPU, five host copies; --saveres copies the whole map and runs numpy.argmax

Both paths ALTERNATE in one process after a warm-up of every shape; the clock is read after a device synchronise.  Per image and path:
  eval     the whole evaluation of the image (backbone included), metrics on the host
  tail     everything after the 1/8-resolution logits (the logits are computed once, outside the clock)
  mask     what --saveres adds: the uint8 mask on the host (readback included, PNG encoding excluded)
  peak     torch.cuda.max_memory_allocated over one evaluation, above what was allocated before it
The kernels' own times come from a separate `rocprofv3 --kernel-trace --stats` run of this script with --kernels N: N alternating launches of
mi_upsample_predict_score and mi_upsample_softmax_multi on the same sources per label size, and nothing else.

    python tools/score_bench.py [--iters 20] [--precision fp32|bf16] [--kernels N]

--classwise measures the confidence histogram of class-wise pseudo-labels (TEST.PSEUDO_CLASSWISE) instead: per label size and source count,
alternating in one process,
  plain    mi_upsample_predict_score with labels (pass 1 without the feature)
  hist     mi_upsample_predict_score_cw with labels and the histogram (pass 1 with it)
  literal  the composition from torch ops: mi_upsample_softmax_multi (the map), max(1), confidence_bin, bincount
on two inputs: the untrained net's logits (confidences spread over many cells) and saturated ones (one class leads by 100 everywhere: every pixel
in ONE cell, the worst case for contention).  A figure is the time per call of --reps back-to-back calls between two device events; with
--kernels N the three run N times each per case and nothing else, for a `rocprofv3 --kernel-trace` run (the kernels' own times).

    python tools/score_bench.py --classwise [--iters 20] [--reps 20] [--precision bf16] [--kernels N]
"""
import argparse
import os
import statistics
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rnd_semantic_segmentation_amd import kernels  # noqa: E402
from rnd_semantic_segmentation_amd.host import metrics, modules, synth  # noqa: E402

SCALES = (0.7, 1.0, 1.3)
NUM_CLASSES = 19
CFG = types.SimpleNamespace(MODEL=types.SimpleNamespace(NUM_CLASSES=NUM_CLASSES))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def literal_score(output, y):
    """ASPPTester.test()'s statements after inference(): the numbers the meters and the matrix receive."""
    pred = output.max(1)[1]
    y0 = y[:1]
    cmt = metrics.confusion_matrix(CFG, torch.flatten(pred), torch.flatten(y0))
    inter, union, target, res = metrics.intersectionAndUnionGPU(pred, y0, NUM_CLASSES, 255)
    return cmt, [t.cpu().numpy() for t in (inter, union, target, res)]


def low_sources(fe, cls, x, multi):
    """The 1/8-resolution logits of every source, as the two tails receive them."""
    with torch.no_grad():
        if not multi:
            lows, flags = cls._lows_multi([fe(x)], [(False,)], "score_bench")
            return lows, flags, (1.0, 1.0)
        sizes, _, div = metrics.multi_scale_plan(x.shape[-2:], True, SCALES)
        feats = [fe(kernels.image_resize_ac(x, hw, with_mirror=True)) for hw in sizes]
        lows, flags = cls._lows_multi(feats, [(False, True)] * len(sizes), "score_bench")
        return lows, flags, (float(div[0]), float(div[1]))


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return (torch.cuda.max_memory_allocated() - base) / 1e6


def event_ms(fn, reps):
    """Milliseconds per call of `reps` back-to-back calls, between two device events."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps


def classwise(args, fe, cls, x):
    K = NUM_CLASSES
    for H, W in ((512, 1024), (1024, 2048)):
        y = torch.from_numpy(synth.synth_label(1, H, W, K, seed=3)).cuda().long()
        for multi in (False, True):
            net, flags, (da, db) = low_sources(fe, cls, x, multi)
            saturated = []
            for low in net:
                m = torch.zeros_like(low)
                m[..., 0] = 100.0
                saturated.append(m)
            for what, lows in (("spread", net), ("saturated", saturated)):
                hist = torch.zeros(K, metrics.PSEUDO_BINS, dtype=torch.int64, device="cuda")

                def plain():
                    return kernels.upsample_predict_score(lows, flags, (H, W), da, db, labels=y[0])

                def with_hist():
                    return kernels.upsample_predict_score(lows, flags, (H, W), da, db, labels=y[0], hist=hist)

                def literal():
                    top = kernels.upsample_softmax_multi(lows, flags, (H, W), da, db).max(1)
                    return torch.bincount((top[1] * metrics.PSEUDO_BINS + metrics.confidence_bin(top[0])).flatten(),
                                          minlength=K * metrics.PSEUDO_BINS).reshape(K, metrics.PSEUDO_BINS)

                fns = (("plain", plain), ("hist", with_hist), ("literal", literal))
                if args.kernels:
                    for _ in range(args.kernels):
                        for _, f in fns:
                            f()
                    torch.cuda.synchronize()
                    continue
                for _, f in fns:                                 # warm-up of every shape
                    f()
                hist.zero_()
                with_hist()
                want = literal()
                same = torch.equal(hist, want)
                cells = int((want > 0).sum())
                times = {name: [] for name, _ in fns}
                for _ in range(args.iters):                      # alternating: drift of the clocks hits all three alike
                    for name, f in fns:
                        times[name].append(event_ms(f, args.reps))
                med = {name: statistics.median(v) for name, v in times.items()}
                print("label %dx%d, %d source%s, %s, %s (%d occupied cells; histogram equals the literal one: %s; %d x %d calls):"
                      % (H, W, len(lows), "s" if len(lows) > 1 else "", args.precision, what, cells, same, args.iters, args.reps))
                for name, _ in fns:
                    v = times[name]
                    print("  %-7s median %8.4f ms per call (min %.4f, max %.4f)   / plain %.3f" % (name, med[name], min(v), max(v), med[name] / med["plain"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--precision", default="fp32", choices=("fp32", "bf16"))
    ap.add_argument("--kernels", type=int, default=0)
    ap.add_argument("--classwise", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    fe = modules.resnet_feature_extractor("resnet101", freeze_bn=True, pretrained_backbone=False)
    cls = modules.ASPP_Classifier_V2(2048, [6, 12, 18, 24], [6, 12, 18, 24], NUM_CLASSES)
    synth.load_formula_weights(fe)
    synth.load_formula_weights(cls)
    fe, cls = fe.cuda().eval().set_precision(args.precision), cls.cuda().eval().set_precision(args.precision)
    x = torch.from_numpy(synth.synth_image(1, 512, 1024, seed=3)).cuda()
    if args.classwise:
        classwise(args, fe, cls, x)
        return
    for H, W in ((512, 1024), (1024, 2048)):
        y = torch.from_numpy(synth.synth_label(1, H, W, NUM_CLASSES, seed=3)).cuda().long()
        for multi in (False, True):
            flip, scales = (True, SCALES) if multi else (False, (1.0,))
            lows, flags, (da, db) = low_sources(fe, cls, x, multi)

            def k_fused():
                return kernels.upsample_predict_score(lows, flags, (H, W), da, db, labels=y[0])

            def k_probs():
                return kernels.upsample_softmax_multi(lows, flags, (H, W), da, db)

            if args.kernels:
                for _ in range(args.kernels):
                    k_fused()
                    k_probs()
                torch.cuda.synchronize()
                continue

            def fused_eval():
                r = metrics.predict_and_score(fe, cls, x, y, flip=flip, scales=scales, num_classes=NUM_CLASSES)
                return r.cmt, [t.numpy() for t in (r.intersection, r.union, r.target, r.output)], r.pred

            def literal_output():
                if multi:
                    return metrics.multi_scale_inference(fe, cls, x, y, flip=True, scales=list(SCALES))
                return metrics.inference(fe, cls, x, y, flip=False)

            def literal_eval():
                output = literal_output()
                return literal_score(output, y) + (output,)

            def fused_tail():
                return metrics.scores_from_counts(k_fused()[2], NUM_CLASSES, None, None)

            def literal_tail():
                return literal_score(k_probs(), y)

            pred_dev, probs_dev = k_fused()[0], k_probs()       # what each path holds on the device when --saveres asks for the mask

            def fused_mask():
                return pred_dev.cpu().numpy()

            def literal_mask():
                return probs_dev.cpu().numpy().squeeze().argmax(0).astype("uint8")

            pairs = {"eval": (fused_eval, literal_eval), "tail": (fused_tail, literal_tail), "mask": (fused_mask, literal_mask)}
            for _ in range(2):                                   # warm-up of every shape of both paths
                for f, l in pairs.values():
                    a, b = f(), l()
            same = torch.equal(fused_eval()[0], literal_eval()[0]) and bool((fused_mask() == literal_mask()).all())
            print("label %dx%d, %s, %s (%d alternating iterations; matrices and masks equal: %s):"
                  % (H, W, "scales 0.7/1.0/1.3 + flip" if multi else "single scale", args.precision, args.iters, same))
            for what, (f, l) in pairs.items():
                n = args.iters if what != "mask" else max(3, args.iters // 4)          # the literal mask runs numpy.argmax on one core
                tf, tl = [], []
                for _ in range(n):                               # alternating: drift of the clocks hits both alike
                    tf.append(timed(f)[0])
                    tl.append(timed(l)[0])
                print("  %-5s fused median %8.3f ms (min %.3f, max %.3f)   literal median %8.3f ms (min %.3f, max %.3f)   literal / fused %.2f"
                      % (what, statistics.median(tf), min(tf), max(tf), statistics.median(tl), min(tl), max(tl),
                         statistics.median(tl) / statistics.median(tf)))
            del pred_dev, probs_dev
            print("  peak  fused %.1f MB   literal %.1f MB (the probability map alone: %.1f MB)"
                  % (peak_of(fused_eval), peak_of(literal_eval), NUM_CLASSES * H * W * 4 / 1e6))


if __name__ == "__main__":
    main()
