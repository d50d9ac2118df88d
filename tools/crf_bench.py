"""The CRF refinement (TEST.CRF): the HIP kernels (mi_crf_refine) against a composition of the same formula from torch ops on the same GPU tensors,
alternating in one process on one MI355X.  K = 19, the default parameters (5 iterations, 7 x 7 window, dilation 4), labels 512 x 1024 and
1024 x 2048; the probabilities are the evaluation tail's output for a synthetic 512 x 1024 image (R101 + ASPP with formula weights), the image is
that picture at the label's size.

  fused    kernels.crf_refine: one init launch, one launch per mean-field iteration (Q tile, image tile and weights in LDS)
  torch    what one would write without it: the 48 weights k(i, o) once per call as [H, W] maps (48 exponentials over the image), then per
           iteration a zero-padded copy of Q and 48 shifted multiply-adds (addcmul_) over the [K, H, W] map, then softmax

Both ALTERNATE after a warm-up of every shape; the clock is read after a device synchronise.  Per size: the whole call, and the time per
iteration = (call with 5 iterations - call with 0) / 5 on each side.  Then the evaluation of the whole image as ASPPTester runs it: the default
path (fused scoring tail), the literal path without the key, and the literal path with the key on.

    python tools/crf_bench.py [--iters 10] [--sizes 512x1024,1024x2048]
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

NUM_CLASSES = 19
CFG = types.SimpleNamespace(MODEL=types.SimpleNamespace(NUM_CLASSES=NUM_CLASSES))
CS = (0.229 * 255, 0.224 * 255, 0.225 * 255)
PAR = dict(iters=5, window=7, dilation=4, pos_w=3.0, pos_xy=3.0, bi_w=10.0, bi_xy=80.0, bi_rgb=13.0)
EPS = 1e-5


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def torch_crf(probs, image, cs, iters, window, dilation, pos_w, pos_xy, bi_w, bi_xy, bi_rgb):
    """The definition of include/mi355seg.h (mi_crf_refine) from torch ops: shifted views of zero-padded tensors."""
    pad = torch.nn.functional.pad
    B, K, H, W = probs.shape
    r = window // 2
    h = r * dilation
    U = torch.log(torch.clamp(probs, min=EPS))
    Q = torch.softmax(U, 1)
    if iters == 0:
        return Q
    scale = torch.tensor(cs, dtype=probs.dtype, device=probs.device).view(1, 3, 1, 1)
    Ip = pad(image * scale, (h, h, h, h))
    inside_p = pad(torch.ones((B, 1, H, W), dtype=probs.dtype, device=probs.device), (h, h, h, h))
    Ic = image * scale
    offsets = [(dy * dilation, dx * dilation) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if (dy, dx) != (0, 0)]
    Np = torch.zeros_like(inside_p[:, :, h:h + H, h:h + W])
    Nb = torch.zeros_like(Np)
    taps = []
    for oy, ox in offsets:
        inside = inside_p[:, :, h + oy:h + oy + H, h + ox:h + ox + W]
        o2 = float(oy * oy + ox * ox)
        gp, gb = torch.exp(torch.tensor(-o2 / (2 * pos_xy ** 2))).item(), torch.exp(torch.tensor(-o2 / (2 * bi_xy ** 2))).item()
        d = Ip[:, :, h + oy:h + oy + H, h + ox:h + ox + W] - Ic
        gc = torch.exp((d * d).sum(1, keepdim=True) * (-1.0 / (2 * bi_rgb ** 2)))
        Np = Np + inside * gp
        Nb = Nb + inside * gb
        taps.append((oy, ox, inside, gp, gb, gc))
    wp = torch.where(Np > 0, pos_w / Np.clamp(min=1e-30), torch.zeros_like(Np))
    wb = torch.where(Nb > 0, bi_w / Nb.clamp(min=1e-30), torch.zeros_like(Nb))
    ks = [(oy, ox, inside * (wp * gp + wb * gb * gc)) for oy, ox, inside, gp, gb, gc in taps]
    del taps
    for _ in range(iters):
        Qp = pad(Q, (h, h, h, h))
        msg = U.clone()
        for oy, ox, k in ks:
            msg.addcmul_(k, Qp[:, :, h + oy:h + oy + H, h + ox:h + ox + W])
        Q = torch.softmax(msg, 1)
    return Q


def literal_score(output, y):
    pred = output.max(1)[1]
    y0 = y[:1]
    cmt = metrics.confusion_matrix(CFG, torch.flatten(pred), torch.flatten(y0))
    inter, union, target, res = metrics.intersectionAndUnionGPU(pred, y0, NUM_CLASSES, 255)
    return cmt, [t.cpu().numpy() for t in (inter, union, target, res)]


def report(name, values):
    return "%s median %9.3f ms (min %.3f, max %.3f)" % (name, statistics.median(values), min(values), max(values))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--sizes", default="512x1024,1024x2048")
    args = ap.parse_args()
    fe = modules.resnet_feature_extractor("resnet101", freeze_bn=True, pretrained_backbone=False)
    cls = modules.ASPP_Classifier_V2(2048, [6, 12, 18, 24], [6, 12, 18, 24], NUM_CLASSES)
    synth.load_formula_weights(fe)
    synth.load_formula_weights(cls)
    fe, cls = fe.cuda().eval().set_precision("fp32"), cls.cuda().eval().set_precision("fp32")
    x = torch.from_numpy(synth.synth_image(1, 512, 1024, seed=3)).cuda()
    for H, W in [tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")]:
        y = torch.from_numpy(synth.synth_label(1, H, W, NUM_CLASSES, seed=3)).cuda().long()
        probs = metrics.inference(fe, cls, x, y, flip=False).contiguous()
        image = x if (H, W) == tuple(x.shape[-2:]) else kernels.image_resize_ac(x, (H, W))
        zero = dict(PAR, iters=0)
        sides = {"fused": (lambda: kernels.crf_refine(probs, image, CS, **PAR).probs, lambda: kernels.crf_refine(probs, image, CS, **zero).probs),
                 "torch": (lambda: torch_crf(probs, image, CS, **PAR), lambda: torch_crf(probs, image, CS, **zero))}
        for _ in range(2):                                       # warm-up of every shape of both sides
            outs = {k: (f(), z()) for k, (f, z) in sides.items()}
        diff = float((outs["fused"][0] - outs["torch"][0]).abs().max())
        moved = float((outs["fused"][0].argmax(1) != probs.argmax(1)).float().mean())
        del outs
        times = {k: ([], []) for k in sides}
        for _ in range(args.iters):                              # alternating: drift of the clocks hits both alike
            for k, (f, z) in sides.items():
                times[k][0].append(timed(f)[0])
                times[k][1].append(timed(z)[0])
        print("label %dx%d, K = %d, 5 iterations, window 7, dilation 4 (%d alternating iterations; max |fused - torch| %.2e; the CRF moves %.1f %% "
              "of the pixels):" % (H, W, NUM_CLASSES, args.iters, diff, 100 * moved))
        per = {}
        for k in sides:
            per[k] = (statistics.median(times[k][0]) - statistics.median(times[k][1])) / PAR["iters"]
            print("  %s   no iteration %9.3f ms   per iteration %9.3f ms" % (report(k + " call", times[k][0]), statistics.median(times[k][1]), per[k]))
        print("  torch / fused: call %.1f, per iteration %.1f" % (statistics.median(times["torch"][0]) / statistics.median(times["fused"][0]),
                                                                  per["torch"] / per["fused"]))

        def eval_default():
            r = metrics.predict_and_score(fe, cls, x, y, flip=False, scales=(1.0,), num_classes=NUM_CLASSES)
            return r.cmt

        def eval_literal():
            return literal_score(metrics.inference(fe, cls, x, y, flip=False), y)[0]

        def eval_crf():
            return literal_score(metrics.crf_refine_output(metrics.inference(fe, cls, x, y, flip=False), x, (H, W), CS, PAR), y)[0]

        evals = {"default (fused scoring, key off)": eval_default, "literal scoring, key off": eval_literal, "literal scoring, TEST.CRF on": eval_crf}
        for _ in range(2):
            for f in evals.values():
                f()
        et = {k: [] for k in evals}
        for _ in range(args.iters):
            for k, f in evals.items():
                et[k].append(timed(f)[0])
        for k in evals:
            print("  whole image, %-34s %s" % (k + ":", report("", et[k])))


if __name__ == "__main__":
    main()
