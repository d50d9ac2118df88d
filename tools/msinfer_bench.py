"""Multi-scale, flip-averaged evaluation timing (reference core/utils/utility.py:193-209; scales [0.7, 1.0, 1.3] with flip) of one 512x1024
image at label sizes 512x1024 and 1024x2048, R101 + ASPP on one MI355X:

  fused        metrics.multi_scale_inference on the engine: mi_image_resize_ac (+ mirror), one batch-2 backbone + head pass per scale,
               ONE mi_upsample_softmax_multi
  composition  the same result from the pieces that existed before: torch bilinear resizes and flips of the input, six
               inference(flip=False) calls (six mi_upsample_softmax launches writing the full tensor), torch adds and two divides

Both variants ALTERNATE in one process after a warm-up of every shape; the clock is read after a device synchronise.  End-to-end ms only: the
backbone passes dominate both.  The tail kernel's own time comes from a separate `rocprofv3 --kernel-trace --stats` run of this script
(--tail-only N runs N fused calls per label size and nothing else).

    python tools/msinfer_bench.py [--iters 20] [--precision fp32|bf16] [--tail-only N]
"""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rnd_semantic_segmentation_amd.host import metrics, modules, synth  # noqa: E402

SCALES = [0.7, 1.0, 1.3]


def composition(fe, cls, image, label):
    """multi_scale_inference written from inference(flip=False) and torch ops, as a user of the package had to before."""
    output = None
    size = image.shape[-2:]
    for s in SCALES:
        x = F.interpolate(image, size=(int(size[0] * s), int(size[1] * s)), mode="bilinear", align_corners=True)
        pred = metrics.inference(fe, cls, x, label, flip=False)
        output = pred if output is None else output + pred
        pred = metrics.inference(fe, cls, torch.flip(x, [3]), label, flip=False)
        output = output + pred.flip(3)
    return output / len(SCALES) / 2


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--precision", default="fp32", choices=("fp32", "bf16"))
    ap.add_argument("--tail-only", type=int, default=0)
    args = ap.parse_args()
    fe = modules.resnet_feature_extractor("resnet101", freeze_bn=True, pretrained_backbone=False)
    cls = modules.ASPP_Classifier_V2(2048, [6, 12, 18, 24], [6, 12, 18, 24], 19)
    synth.load_formula_weights(fe)
    synth.load_formula_weights(cls)
    fe, cls = fe.cuda().eval().set_precision(args.precision), cls.cuda().eval().set_precision(args.precision)
    x = torch.from_numpy(synth.synth_image(1, 512, 1024, seed=3)).cuda()
    for H, W in ((512, 1024), (1024, 2048)):
        label = torch.zeros((1, H, W), dtype=torch.int64, device="cuda")

        def fused():
            return metrics.multi_scale_inference(fe, cls, x, label, flip=True, scales=SCALES)

        def comp():
            with torch.no_grad():
                return composition(fe, cls, x, label)

        if args.tail_only:
            for _ in range(args.tail_only):
                fused()
            torch.cuda.synchronize()
            continue
        for _ in range(3):                                   # warm-up of every shape of both variants
            a, b = fused(), comp()
        torch.cuda.synchronize()
        diff = (a - b).abs().max().item()
        tf, tc = [], []
        for _ in range(args.iters):                          # alternating: drift of the clocks hits both alike
            tf.append(timed(fused)[0])
            tc.append(timed(comp)[0])
        out_mb = 19 * H * W * 4 / 1e6
        print("label %dx%d (%s, %d alternating iterations, output %.1f MB; max |fused - composition| %.1e):" % (H, W, args.precision, args.iters, out_mb, diff))
        for name, t in (("fused", tf), ("composition", tc)):
            print("  %-12s end to end: median %.2f ms, min %.2f ms, max %.2f ms" % (name, statistics.median(t), min(t), max(t)))
        print("  end-to-end median ratio composition / fused: %.3f" % (statistics.median(tc) / statistics.median(tf)))


if __name__ == "__main__":
    main()
