"""The curve tail (TEST.CURVES): the HIP kernel (mi_upsample_curves) against the literal composition (the materialised probability map of
mi_upsample_softmax_multi through metrics.literal_curves) on the same GPU tensors, with the plain evaluation tail (mi_upsample_predict_score)
beside them, alternating in one process on one MI355X.  K = 19, labels 512 x 1024 and 1024 x 2048, one source and six (three scales, each
plain and mirrored), on two inputs:

  net         the 1/8-resolution logits of R101 + ASPP with formula weights on a synthetic 512 x 1024 picture (an untrained net: spread values)
  saturated   one class leads by a logit margin of 100 everywhere: every add falls into the two cells per class the ballots aggregate

All sides ALTERNATE after a warm-up of every shape; the clock is read after a device synchronise (around 10 fused calls in a row, divided by
10); the histograms are compared first.  Then ASPPTester.test() itself (R101 + ASPP with formula weights, 8 pictures of 512 x 1024 per call,
fp32, the default fused scoring tail) with the key off and on, alternating, per picture.  The byte floor of the call is printed beside the
times: the label (8 bytes per pixel) plus the low-resolution logits.

    python tools/curves_bench.py [--iters 5] [--sizes 512x1024,1024x2048]
    python tools/curves_bench.py --kernels 20 --case net --sources 6 --sizes 1024x2048      # the fused call and, as a yardstick, the plain evaluation tail, each N times, for a rocprofv3 --kernel-trace --stats run
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rnd_semantic_segmentation_amd import kernels  # noqa: E402
from rnd_semantic_segmentation_amd.host import metrics, modules, synth  # noqa: E402

NUM_CLASSES = 19
ECE_BINS = 15
FUSED_REPS = 10             # fused calls per clock reading: one call is one launch long, the clock's own cost would show
HBM_MEASURED = 6.29e12      # bytes / s of a float4 copy on this part (the figure DESIGN.md uses for every floor)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def report(name, values):
    return "%s median %9.3f ms (min %.3f, max %.3f)" % (name, statistics.median(values), min(values), max(values))


def net_sources():
    """(one source, six sources): the logits of the untrained net on one synthetic picture at scale 1, and at 0.7 / 1.0 / 1.3 plain and mirrored."""
    fe = modules.resnet_feature_extractor("resnet101", freeze_bn=True, pretrained_backbone=False)
    cls = modules.ASPP_Classifier_V2(2048, [6, 12, 18, 24], [6, 12, 18, 24], NUM_CLASSES)
    synth.load_formula_weights(fe)
    synth.load_formula_weights(cls)
    for m in (fe, cls):
        m.cuda().eval()
        if hasattr(m, "set_precision"):
            m.set_precision("fp32")
    x = torch.from_numpy(synth.synth_image(1, 512, 1024, seed=3)).cuda()
    sizes, _, divisors = metrics.multi_scale_plan(x.shape[-2:], True, (0.7, 1.0, 1.3))
    with torch.no_grad():
        feats = [fe(kernels.image_resize_ac(x, hw, with_mirror=True)) for hw in sizes]
        lows, flags = cls._lows_multi(feats, [(False, True)] * len(sizes), "curves_bench")
        one = cls._lows_multi([fe(x)], [(False,)], "curves_bench")[0]
    lows = [low.contiguous().clone() for low in lows]
    return ([one[0].contiguous().clone()], [False], 1.0, 1.0), (lows, flags, float(divisors[0]), float(divisors[1]))


def saturated_sources(like):
    lows = []
    for low in like[0]:
        m = torch.zeros_like(low)
        m[..., 7] = 100.0
        lows.append(m)
    return (lows,) + tuple(like[1:])


def buffers():
    return (torch.zeros(NUM_CLASSES, metrics.CURVE_BINS, 2, dtype=torch.int64, device="cuda"),
            torch.zeros(ECE_BINS, 3, dtype=torch.int64, device="cuda"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--sizes", default="512x1024,1024x2048")
    ap.add_argument("--images", type=int, default=8, help="pictures per ASPPTester.test() call of the last section")
    ap.add_argument("--kernels", type=int, default=0, help="run the fused call and the plain evaluation tail this many times each on one input and exit (for a kernel trace)")
    ap.add_argument("--case", default="net", choices=("net", "saturated"))
    ap.add_argument("--sources", type=int, default=1, choices=(1, 6))
    args = ap.parse_args()
    sizes = [tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")]
    one, six = net_sources()
    cases = {("net", 1): one, ("net", 6): six, ("saturated", 1): saturated_sources(one), ("saturated", 6): saturated_sources(six)}
    if args.kernels:
        H, W = sizes[0]
        src = cases[(args.case, args.sources)]
        lab = torch.from_numpy(synth.synth_label(1, H, W, NUM_CLASSES, seed=3))[0].cuda().long().contiguous()
        pr, cal = buffers()
        for _ in range(args.kernels):
            kernels.upsample_curves(src[0], src[1], (H, W), src[2], src[3], lab, pr=pr, cal=cal)
            kernels.upsample_predict_score(src[0], src[1], (H, W), src[2], src[3], labels=lab)
        torch.cuda.synchronize()
        print("%s, %d source(s), %dx%d: %d calls, %d pixels counted per call" % (args.case, args.sources, H, W, args.kernels,
                                                                               int(cal[:, 0].sum()) // args.kernels))
        return
    for H, W in sizes:
        lab = torch.from_numpy(synth.synth_label(1, H, W, NUM_CLASSES, seed=3))[0].cuda().long().contiguous()
        for (case, n), src in cases.items():
            pr, cal = buffers()
            low_bytes = sum(low.numel() * 4 for low in src[0])
            floor = (H * W * 8 + low_bytes) / HBM_MEASURED * 1e3

            def fused():
                return kernels.upsample_curves(src[0], src[1], (H, W), src[2], src[3], lab, pr=pr, cal=cal)

            def literal():
                return metrics.literal_curves(kernels.upsample_softmax_multi(src[0], src[1], (H, W), src[2], src[3]), lab[None], NUM_CLASSES, ECE_BINS)

            def score():
                return kernels.upsample_predict_score(src[0], src[1], (H, W), src[2], src[3], labels=lab)

            sides = {"fused": fused, "literal": literal, "predict_score": score}
            reps = {"fused": FUSED_REPS, "literal": 1, "predict_score": FUSED_REPS}
            for _ in range(2):                                   # warm-up of every shape of every side
                pr.zero_()
                cal.zero_()
                outs = {k: f() for k, f in sides.items()}
            same = bool(torch.equal(outs["fused"][0], outs["literal"][0]) and torch.equal(outs["fused"][1], outs["literal"][1]))
            assert same, "the fused histograms differ from the literal composition"
            table = metrics.curves_summary(outs["literal"][0], outs["literal"][1])
            low_cells = int(outs["literal"][0][:, 0, 0].sum() + outs["literal"][0][:, 255, 1].sum())
            total = int(outs["literal"][0].sum())
            del outs
            times = {k: [] for k in sides}
            for _ in range(args.iters):                          # alternating: drift of the clocks hits all alike
                for k, f in sides.items():
                    times[k].append(timed(lambda: [f() for _ in range(reps[k])])[0] / reps[k])
            print("label %dx%d, K = %d, %s, %d source(s) (%d alternating iterations; histograms EQUAL; %.1f %% of the adds in the ballot cells; "
                  "mAP %.4f, ECE %.4f):" % (H, W, NUM_CLASSES, case, n, args.iters, 100.0 * low_cells / total,
                                            float("nan") if table["map"] is None else table["map"], table["calibration"]["ece"]))
            for k in sides:
                print("  " + report("%-14s call" % k, times[k]))
            print("  literal / fused: %.1f;  fused / predict_score: %.2f;  byte floor of the call (%d bytes at %.2f TB/s): %.4f ms, the fused call is "
                  "%.1f x that" % (statistics.median(times["literal"]) / statistics.median(times["fused"]),
                                   statistics.median(times["fused"]) / statistics.median(times["predict_score"]), H * W * 8 + low_bytes,
                                   HBM_MEASURED / 1e12, floor, statistics.median(times["fused"]) / floor))
    del cases, one, six
    tester_times(sizes, args.iters, args.images)


class _Quiet:
    def info(self, s):
        pass

    warning = info


def tester_times(sizes, iters, images):
    """ASPPTester.test() itself over a loader of `images` pictures (a list of CPU batches, as a DataLoader yields them), key off and on
    alternating: the host-to-device copies of picture and label, the evaluation, with the key on the extra launch, and once per call the
    summary lines and the JSON files.  Printed per picture: the time of the call / images."""
    import tempfile
    from rnd_semantic_segmentation_amd.host.config import cfg as base
    from rnd_semantic_segmentation_amd.host.tester import ASPPTester

    class Tester(ASPPTester):
        build_feature_extractor = staticmethod(lambda cfg: modules.resnet_feature_extractor("resnet101", freeze_bn=True, pretrained_backbone=False))

    x = torch.from_numpy(synth.synth_image(1, 512, 1024, seed=3))
    names = {i: "class%d" % i for i in range(NUM_CLASSES)}
    with tempfile.TemporaryDirectory() as out:
        for H, W in sizes:
            y = torch.from_numpy(synth.synth_label(1, H, W, NUM_CLASSES, seed=3))
            loader = [(x, y, ("picture%d" % i,)) for i in range(images)]
            testers = {}
            for key in (False, True):
                cfg = base.clone()
                cfg.defrost()
                cfg.merge_from_list(["MODEL.NUM_CLASSES", NUM_CLASSES, "MODEL.FREEZE_BN", True, "OUTPUT_DIR", out, "TEST.CURVES", key])
                t = Tester(cfg, torch.device("cuda"), loader, _Quiet(), [0] * 768, names, saveres=False)
                synth.load_formula_weights(t.feature_extractor)
                synth.load_formula_weights(t.classifier)
                testers["TEST.CURVES on" if key else "TEST.CURVES off"] = t
            cmts = {k: t.test() for k, t in testers.items()}                     # warm-up of both
            same = bool(torch.equal(cmts["TEST.CURVES off"], cmts["TEST.CURVES on"]))
            et = {k: [] for k in testers}
            for _ in range(iters):
                for k, t in testers.items():
                    et[k].append(timed(t.test)[0] / images)
            print("ASPPTester.test() per picture, fp32, %d pictures of 512x1024 per call, label %dx%d (%d alternating calls; confusion matrices %s):"
                  % (images, H, W, iters, "EQUAL" if same else "DIFFER"))
            for k in testers:
                print("  %-20s %s" % (k + ":", report("", et[k])))
            del testers


if __name__ == "__main__":
    main()
