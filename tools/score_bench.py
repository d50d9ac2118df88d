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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--precision", default="fp32", choices=("fp32", "bf16"))
    ap.add_argument("--kernels", type=int, default=0)
    args = ap.parse_args()
    fe = modules.resnet_feature_extractor("resnet101", freeze_bn=True, pretrained_backbone=False)
    cls = modules.ASPP_Classifier_V2(2048, [6, 12, 18, 24], [6, 12, 18, 24], NUM_CLASSES)
    synth.load_formula_weights(fe)
    synth.load_formula_weights(cls)
    fe, cls = fe.cuda().eval().set_precision(args.precision), cls.cuda().eval().set_precision(args.precision)
    x = torch.from_numpy(synth.synth_image(1, 512, 1024, seed=3)).cuda()
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
