"""The surface-distance tail (TEST.SURFACE_METRICS): the fused kernels (mi_surface_score) against what a user has without them, alternating in one
process on one MI355X.  Masks are 352 x 352 (PraNet's test size) and 1072 x 1920 (the largest Kvasir pictures), B = 1 and 16.

  fused    kernels.surface_score (seven launches for the whole batch), one device-to-host copy of the 27 integers and 2 sums per image, and
           host/metrics.py surface_image_stats per image
  literal  host/metrics.py literal_surface_stats per image: surfaces from shifted comparisons, torch.cdist in chunks, min, sort - on the GPU
  scipy    the host path: both maps copied to the host, binary_erosion and two distance_transform_edt per image (medpy's hd / hd95 / assd)

Three inputs: `compact` = two overlapping ellipses of about a sixth of the picture (what a trained net and its label look like), `shifted` = two
large ellipses shifted against each other (long perimeters, large distances), `speckle` = compact with 3 % of the pixels flipped (the worst case
for the number of surface pixels).  A figure is the median wall time of one call over the whole batch, the clock read after a device
synchronise; a path that takes long runs fewer times (at least twice; the count is printed), and one that would need more than 20 s for
a batch, judged from one image, is not run on it (the row says so).  The byte floor is the label and mask bytes
(9 per pixel) over 4 TB/s.  --kernels N runs the fused tail N times per case and nothing else, for a `rocprofv3 --kernel-trace --stats` run (the
seven kernels' own times).  --tester times PranetTester.test() on a stub net with the key off and on, alternating.

    python tools/surface_bench.py [--iters 20] [--tester] [--kernels N] [--case compact] [--size 1072x1920] [--batch 16]
"""
import argparse
import logging
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rnd_semantic_segmentation_amd import kernels  # noqa: E402
from rnd_semantic_segmentation_amd.host import config as hc, metrics, pranet  # noqa: E402

SIZES = ((352, 352), (1072, 1920))
BATCHES = (1, 16)
INPUTS = ("compact", "shifted", "speckle")
TOLERANCES = (2.0,)
HBM_BYTES_PER_S = 4e12
SLOW_BUDGET_S = 4.0          # a path stops being repeated once it has used this much
SKIP_S = 20.0                # a path is not run on a batch that would take longer than this per call, judged from one image


def ellipse(H, W, cy, cx, ry, rx):
    yy, xx = np.mgrid[0:H, 0:W]
    return (((yy - cy * H) / (ry * H)) ** 2 + ((xx - cx * W) / (rx * W)) ** 2) < 1


def make(kind, B, H, W):
    """(pred uint8 [B,H,W], labels int64 [B,H,W]) on the GPU; image b is shifted by b pixels so that the images of a batch differ."""
    g = np.random.RandomState(17)
    pred, lab = np.zeros((B, H, W), np.uint8), np.zeros((B, H, W), np.int64)
    for b in range(B):
        if kind == "shifted":
            p, t = ellipse(H, W, 0.45, 0.40, 0.40, 0.35), ellipse(H, W, 0.55, 0.60, 0.40, 0.35)
        else:
            p, t = ellipse(H, W, 0.50, 0.50, 0.22, 0.20), ellipse(H, W, 0.52, 0.48, 0.20, 0.23)
        if kind == "speckle":
            p, t = p ^ (g.rand(H, W) < 0.03), t ^ (g.rand(H, W) < 0.03)
        pred[b], lab[b] = np.roll(p, b, 1), np.roll(t, b, 0)
    return torch.from_numpy(pred).cuda(), torch.from_numpy(lab).cuda()


def fused(pred, lab):
    r = kernels.surface_score(pred, lab, 1, 95, TOLERANCES)
    ints, sums = r.ints.cpu().numpy(), r.sums.cpu().numpy()
    return [metrics.surface_image_stats(ints[b], sums[b], TOLERANCES, 95) for b in range(pred.shape[0])]


def literal(pred, lab):
    return [metrics.literal_surface_stats(pred[b], lab[b], 1, 95, TOLERANCES) for b in range(pred.shape[0])]


def host_scipy(pred, lab):
    from scipy import ndimage as ndi
    cross = ndi.generate_binary_structure(2, 1)
    P, G = pred.cpu().numpy() == 1, lab.cpu().numpy() == 1
    out = []
    for b in range(P.shape[0]):
        sp, sg = P[b] & ~ndi.binary_erosion(P[b], cross, border_value=0), G[b] & ~ndi.binary_erosion(G[b], cross, border_value=0)
        a, c = ndi.distance_transform_edt(~sg)[sp], ndi.distance_transform_edt(~sp)[sg]
        both = np.hstack([a, c])
        out.append({"HD": float(both.max()), "HD95": float(np.percentile(both, 95)), "ASSD": float((a.mean() + c.mean()) / 2),
                    "NSD@2": float((both <= 2.0).mean()), "defined": True})
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def bench(iters, inputs, sizes, batches):
    try:
        import scipy  # noqa: F401
        paths = (("fused", fused), ("literal", literal), ("scipy", host_scipy))
    except ImportError:
        paths = (("fused", fused), ("literal", literal))
        print("scipy is not importable: the host path is not measured")
    print("%-8s %-11s %3s | %10s %5s | %10s %5s | %10s %5s | %9s %7s | %8s %8s | %s" % (
        "input", "size", "B", "fused ms", "runs", "literal ms", "runs", "scipy ms", "runs", "floor us", "x floor", "|S(P)|", "|S(G)|", "agreement"))
    for kind in inputs:
        for H, W in sizes:
            for B in batches:
                pred, lab = make(kind, B, H, W)
                run = []
                for n, fn in paths:                                    # a path that needs more than SKIP_S for one image is not run on sixteen
                    one = timed(lambda: fn(pred[:1], lab[:1]))[0] if n != "fused" else 0.0
                    if one * B > SKIP_S * 1e3:
                        print("%-8s %-11s %3d | %s not run: one image took %.1f s" % (kind, "%dx%d" % (H, W), B, n, one / 1e3), flush=True)
                    else:
                        run.append((n, fn))
                times, outs = {n: [] for n, _ in run}, {}
                for n, fn in run:                                      # warm-up of this shape, every path
                    outs[n] = timed(lambda: fn(pred, lab))[1]
                for i in range(iters):                                 # alternating
                    for n, fn in run:
                        if i < 2 or sum(times[n]) < SLOW_BUDGET_S * 1e3:
                            times[n].append(timed(lambda: fn(pred, lab))[0])
                gaps = []
                for n in outs:
                    if n != "fused":
                        gaps.append("%s %.1e" % (n, max(abs(a[k] - b[k]) / max(abs(a[k]), 1.0) for a, b in zip(outs["fused"], outs[n])
                                                      for k in ("HD", "HD95", "ASSD", "NSD@2"))))
                floor_us = B * H * W * 9 / HBM_BYTES_PER_S * 1e6
                med = {n: statistics.median(times[n]) for n in times}
                ints = kernels.surface_score(pred, lab, 1, 95, TOLERANCES).ints[0].tolist()
                cols = "".join(" %10.3f %5d |" % (med[n], len(times[n])) if n in med else " %10s %5s |" % ("-", "-") for n in ("fused", "literal", "scipy"))
                print("%-8s %-11s %3d |%s %9.1f %7.1f | %8d %8d | gap to fused: %s" % (
                    kind, "%dx%d" % (H, W), B, cols, floor_us, med["fused"] * 1e3 / floor_us, ints[2], ints[3], ", ".join(gaps)), flush=True)


def kernels_only(n, inputs, sizes, batches):
    for kind in inputs:
        for H, W in sizes:
            for B in batches:
                pred, lab = make(kind, B, H, W)
                for _ in range(n):
                    kernels.surface_score(pred, lab, 1, 95, TOLERANCES)
                torch.cuda.synchronize()
                print("ran", kind, H, W, B, n, flush=True)


class _Stub(torch.nn.Module):
    def __init__(self, maps):
        super().__init__()
        self.maps = maps

    def forward(self, x):
        return (self.maps, self.maps, self.maps, self.maps)


def tester_cost(iters):
    """PranetTester.test() on a stub net (no backbone: the tail alone) over 8 batches of B images, key off and on, alternating."""
    log = logging.getLogger("surface_bench")
    log.addHandler(logging.NullHandler())
    log.propagate = False
    print("%-11s %3s %6s | %10s %10s | %s" % ("size", "B", "polyp", "off ms", "on ms", "cost of the key per image, us"))
    for H, W in SIZES:
        for B in BATCHES:
            for polyp in (False, True):
                _, lab = make("compact", B, H, W)
                low = 8.0 * ellipse(352, 352, 0.5, 0.5, 0.22, 0.2) - 4.0 + 0.3 * np.random.RandomState(3).randn(B, 1, 352, 352)
                maps = torch.from_numpy(low.astype(np.float32)).cuda()
                loader = [(torch.zeros(B, 3, 8, 8), lab.cpu(), ["im%d" % i for i in range(B)])] * 8
                testers = {}
                for on in (False, True):
                    cfg = hc.CfgNode(hc.default_tree())
                    cfg.merge_from_list(["MODEL.NUM_CLASSES", 2, "OUTPUT_DIR", tempfile.mkdtemp(), "TEST.POLYP_METRICS", polyp, "TEST.SURFACE_METRICS", on])
                    cfg.freeze()
                    t = pranet.PranetTester(cfg, torch.device("cuda"), loader, log)
                    t.model = _Stub(maps)
                    t.test()
                    testers[on] = t
                times = {False: [], True: []}
                for _ in range(iters):
                    for on in (False, True):
                        times[on].append(timed(testers[on].test)[0])
                off, on_ms = statistics.median(times[False]), statistics.median(times[True])
                print("%-11s %3d %6s | %10.3f %10.3f | %.1f" % ("%dx%d" % (H, W), B, polyp, off, on_ms, (on_ms - off) * 1e3 / (8 * B)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--kernels", type=int, default=0)
    ap.add_argument("--tester", action="store_true")
    ap.add_argument("--case", choices=INPUTS, default=None, help="one input only")
    ap.add_argument("--size", default=None, help="one size only, HxW")
    ap.add_argument("--batch", type=int, default=None, help="one batch size only")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "surface_bench needs the MI355X"
    sel = ((a.case,) if a.case else INPUTS, (tuple(int(v) for v in a.size.split("x")),) if a.size else SIZES, (a.batch,) if a.batch else BATCHES)
    if a.kernels:
        kernels_only(a.kernels, *sel)
    elif a.tester:
        tester_cost(a.iters)
    else:
        bench(a.iters, *sel)


if __name__ == "__main__":
    main()
