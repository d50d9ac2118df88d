"""The boundary metrics (TEST.BOUNDARY): the HIP kernel pair (mi_boundary_score) against the literal composition from torch ops
(metrics.literal_boundary_histograms: the masks of all classes eroded D times by max_pool2d, for both class maps) on the same GPU tensors,
alternating in one process on one MI355X.  K = 19, labels 512 x 1024 and 1024 x 2048 at the 2 % width (23 and 46), on two inputs:

  blocks    a block-structured label map (cells of H / 12 pixels, an ignored border band) with a copy shifted by (3, 5) as the prediction
  uniform   one class everywhere: every interior pixel walks to the cap and lands in one cell (the column pass's worst case)

Both sides ALTERNATE after a warm-up of every shape; the clock is read after a device synchronise (around 10 fused calls in a row, divided
by 10: one call is two launches); the histograms are compared first.  Then
ASPPTester.test() itself (R101 + ASPP with formula weights, 8 pictures of 512 x 1024 per call, fp32, the default fused scoring tail) with the
key off and on, alternating, per picture: copies to the device, evaluation, counting, and the call's summary lines and JSON files.  The byte floor of the call is printed beside the times: 9 bytes per pixel read (label and mask) plus the
workspace word written and read back (8 bytes).

    python tools/boundary_bench.py [--iters 5] [--sizes 512x1024,1024x2048]
    python tools/boundary_bench.py --kernels 20 --case blocks --sizes 1024x2048      # the fused call alone, for a rocprofv3 --kernel-trace --stats run
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rnd_semantic_segmentation_amd import kernels  # noqa: E402
from rnd_semantic_segmentation_amd.host import metrics, modules, synth  # noqa: E402

NUM_CLASSES = 19
FUSED_REPS = 10             # fused calls per clock reading: one call is a few launches long, the clock's own cost would show
HBM_MEASURED = 6.29e12      # bytes / s of a float4 copy on this part (the figure DESIGN.md uses for every floor)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def block_inputs(H, W, seed=3):
    rng = np.random.RandomState(seed)
    cell = max(4, min(H, W) // 12)
    grid = rng.randint(0, NUM_CLASSES, size=(-(-H // cell), -(-W // cell)))
    lab = np.repeat(np.repeat(grid, cell, axis=0), cell, axis=1)[:H, :W].astype(np.int64)
    border = max(1, min(H, W) // 24)
    pred = np.roll(lab, (3, 5), axis=(0, 1)).astype(np.uint8)
    lab[:border] = lab[-border:] = 255
    lab[:, :border] = lab[:, -border:] = 255
    return torch.from_numpy(pred).cuda(), torch.from_numpy(lab).cuda()


def uniform_inputs(H, W):
    return torch.full((H, W), 7, dtype=torch.uint8, device="cuda"), torch.full((H, W), 7, dtype=torch.int64, device="cuda")


def report(name, values):
    return "%s median %9.3f ms (min %.3f, max %.3f)" % (name, statistics.median(values), min(values), max(values))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--sizes", default="512x1024,1024x2048")
    ap.add_argument("--images", type=int, default=8, help="pictures per ASPPTester.test() call of the last section")
    ap.add_argument("--kernels", type=int, default=0, help="run the fused call this many times on one input and exit (for a kernel trace)")
    ap.add_argument("--case", default="blocks", choices=("blocks", "uniform"))
    args = ap.parse_args()
    sizes = [tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")]
    if args.kernels:
        H, W = sizes[0]
        D = metrics.boundary_width((H, W))
        pred, lab = block_inputs(H, W) if args.case == "blocks" else uniform_inputs(H, W)
        hist = torch.zeros(5, NUM_CLASSES, D + 1, dtype=torch.int64, device="cuda")
        for _ in range(args.kernels):
            kernels.boundary_score(pred, lab, NUM_CLASSES, 255, D, hist)
        torch.cuda.synchronize()
        print("%s %dx%d, D %d: %d calls, %d pixels counted per call" % (args.case, H, W, D, args.kernels, int(hist[0].sum()) // args.kernels))
        return
    for H, W in sizes:
        D = metrics.boundary_width((H, W))
        floor = H * W * (9 + 8) / HBM_MEASURED * 1e3
        for case, (pred, lab) in (("blocks", block_inputs(H, W)), ("uniform", uniform_inputs(H, W))):
            hist = torch.zeros(5, NUM_CLASSES, D + 1, dtype=torch.int64, device="cuda")
            sides = {"fused": lambda: kernels.boundary_score(pred, lab, NUM_CLASSES, 255, D, hist),
                     "torch": lambda: metrics.literal_boundary_histograms(pred, lab, NUM_CLASSES, 255, D)}
            reps = {"fused": FUSED_REPS, "torch": 1}
            for _ in range(2):                                   # warm-up of every shape of both sides
                hist.zero_()
                outs = {k: f() for k, f in sides.items()}
            same = bool(torch.equal(outs["fused"], outs["torch"]))
            band = int(outs["torch"][0, :, :D].sum())
            total = int(outs["torch"][0].sum())
            table = metrics.boundary_summary(outs["torch"].cpu(), [D])
            del outs
            times = {k: [] for k in sides}
            for _ in range(args.iters):                          # alternating: drift of the clocks hits both alike
                for k, f in sides.items():
                    times[k].append(timed(lambda: [f() for _ in range(reps[k])])[0] / reps[k])
            print("label %dx%d, K = %d, width %d, %s (%d alternating iterations; histograms %s; %.1f %% of the labelled pixels in the band; mean "
                  "Boundary IoU %.4f, trimap IoU %.4f):" % (H, W, NUM_CLASSES, D, case, args.iters, "EQUAL" if same else "DIFFER", 100.0 * band / total,
                                                            table["mean_boundary_iou"][0], table["mean_trimap_iou"][0]))
            for k in sides:
                print("  " + report(k + " call", times[k]))
            print("  torch / fused: %.0f;  byte floor of the call (17 bytes per pixel at %.2f TB/s): %.4f ms, the fused call is %.1f x that"
                  % (statistics.median(times["torch"]) / statistics.median(times["fused"]), HBM_MEASURED / 1e12, floor,
                     statistics.median(times["fused"]) / floor))
    tester_times(sizes, args.iters, args.images)


class _Quiet:
    def info(self, s):
        pass

    warning = info


def tester_times(sizes, iters, images):
    """ASPPTester.test() itself over a loader of `images` pictures (a list of CPU batches, as a DataLoader yields them), key off and on
    alternating: the host-to-device copies of picture and label, the evaluation, with the key on the counting, and once per call the
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
                cfg.merge_from_list(["MODEL.NUM_CLASSES", NUM_CLASSES, "MODEL.FREEZE_BN", True, "OUTPUT_DIR", out, "TEST.BOUNDARY", key])
                t = Tester(cfg, torch.device("cuda"), loader, _Quiet(), [0] * 768, names, saveres=False)
                synth.load_formula_weights(t.feature_extractor)
                synth.load_formula_weights(t.classifier)
                testers["TEST.BOUNDARY on" if key else "TEST.BOUNDARY off"] = t
            cmts = {k: t.test() for k, t in testers.items()}                     # warm-up of both
            same = bool(torch.equal(cmts["TEST.BOUNDARY off"], cmts["TEST.BOUNDARY on"]))
            et = {k: [] for k in testers}
            for _ in range(iters):
                for k, t in testers.items():
                    et[k].append(timed(t.test)[0] / images)
            print("ASPPTester.test() per picture, fp32, %d pictures of 512x1024 per call, label %dx%d, width %d (%d alternating calls; confusion "
                  "matrices %s):" % (images, H, W, testers["TEST.BOUNDARY on"].boundary_widths[-1], iters, "EQUAL" if same else "DIFFER"))
            for k in testers:
                print("  %-20s %s" % (k + ":", report("", et[k])))
            del testers


if __name__ == "__main__":
    main()
