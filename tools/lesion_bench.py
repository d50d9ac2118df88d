"""The lesion-wise tail (TEST.LESION_METRICS, TEST.MASK_MIN_AREA): the union-find kernels (mi_lesion_score) against what a user has without them,
alternating in one process on one MI355X.  Masks are 352 x 352 (PraNet's test size) and 1072 x 1920 (the largest Kvasir pictures), B = 1 and 16.

  fused    kernels.lesion_score (a memset and seven launches for the whole batch), one device-to-host copy of the 12 integers per image, and
           host/metrics.py lesion_image_stats per image; the filtered mask stays on the device
  literal  host/metrics.py literal_lesion_stats per image: minimum-index propagation by max_pool2d until nothing changes, bincount - on the GPU
  scipy    the host path: both maps copied to the host, scipy.ndimage.label and np.bincount per image, the filtered mask copied back

Three inputs: `compact` = two overlapping ellipses of about a sixth of the picture (what a trained net and its label look like), `speckle` =
compact with 3 % of the pixels flipped (thousands of components), `spiral` = a one-pixel-wide spiral filling the picture against the compact label
(one component whose pixels are all run starts of length one on its vertical strokes: union-find's longest parent chains, and as many rounds of
the literal path as the spiral has pixels).  A figure is the median wall time of one call over the whole batch, the clock read after a device
synchronise; a path that takes long runs fewer times (at least twice; the count is printed), and one that would need more than 20 s for a
batch, judged from one image, is not run on it (the row says so).  The byte floor is the mask and label bytes read plus the filtered mask
written (10 per pixel) over 4 TB/s.  --kernels N runs the fused tail N times per case and nothing else, for a `rocprofv3 --kernel-trace --stats`
run (the kernels' own times).  --tester times PranetTester.test() on a stub net with the keys off and on, alternating.

    python tools/lesion_bench.py [--iters 20] [--tester] [--kernels N] [--case spiral] [--size 1072x1920] [--batch 16]
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
INPUTS = ("compact", "speckle", "spiral")
SETTINGS = dict(connectivity=8, min_area=64, keep_largest=False, overlap=0.0)
HBM_BYTES_PER_S = 4e12
SLOW_BUDGET_S = 4.0          # a path stops being repeated once it has used this much
SKIP_S = 20.0                # a path is not run on a batch that would take longer than this per call, judged from one image
LITERAL_MAX_ROUNDS = 70000   # the literal path gives up beyond this many propagation rounds: the 352 x 352 spiral (62 303 pixels) still runs


def ellipse(H, W, cy, cx, ry, rx):
    yy, xx = np.mgrid[0:H, 0:W]
    return (((yy - cy * H) / (ry * H)) ** 2 + ((xx - cx * W) / (rx * W)) ** 2) < 1


def spiral(H, W):
    """A one-pixel-wide spiral from pixel 0 inwards: concentric rings two pixels apart, each opened below its top-left corner and tied to the
    next ring's top row."""
    m = np.zeros((H, W), bool)
    for o in range(0, (min(H, W) - 1) // 2, 2):
        m[o, o:W - o] = m[H - 1 - o, o:W - o] = True
        m[o:H - o, o] = m[o:H - o, W - 1 - o] = True
        m[o + 1, o] = False
        if o + 2 < min(H, W) - 1 - (o + 2):
            m[o + 2, o + 1] = True
    return m


def make(kind, B, H, W):
    """(pred uint8 [B,H,W], labels int64 [B,H,W]) on the GPU; image b is shifted by b pixels so that the images of a batch differ."""
    g = np.random.RandomState(17)
    pred, lab = np.zeros((B, H, W), np.uint8), np.zeros((B, H, W), np.int64)
    for b in range(B):
        p, t = ellipse(H, W, 0.50, 0.50, 0.22, 0.20), ellipse(H, W, 0.52, 0.48, 0.20, 0.23)
        if kind == "speckle":
            p, t = p ^ (g.rand(H, W) < 0.03), t ^ (g.rand(H, W) < 0.03)
        if kind == "spiral":
            pred[b], lab[b] = spiral(H, W), np.roll(t, b, 0)           # a shifted spiral is no spiral: only the label moves
        else:
            pred[b], lab[b] = np.roll(p, b, 1), np.roll(t, b, 0)
    return torch.from_numpy(pred).cuda(), torch.from_numpy(lab).cuda()


def fused(pred, lab):
    r = kernels.lesion_score(pred, lab, 1, **SETTINGS)
    ints = r.ints.cpu().numpy()
    return [metrics.lesion_image_stats(ints[b]) for b in range(pred.shape[0])], r.filtered


def literal(pred, lab):
    out = [metrics.literal_lesion_stats(pred[b], lab[b], 1, SETTINGS["connectivity"], SETTINGS["min_area"], SETTINGS["keep_largest"], SETTINGS["overlap"],
                                        max_rounds=LITERAL_MAX_ROUNDS) for b in range(pred.shape[0])]
    return [metrics.lesion_image_stats(i) for i, _ in out], torch.stack([f for _, f in out])


def host_scipy(pred, lab):
    from scipy import ndimage as ndi
    full = ndi.generate_binary_structure(2, 2)
    P, G = pred.cpu().numpy() == 1, lab.cpu().numpy() == 1
    stats, filtered = [], np.zeros(P.shape, np.uint8)
    for b in range(P.shape[0]):
        lp, n_p = ndi.label(P[b], structure=full)
        lg, n_g = ndi.label(G[b], structure=full)
        area_p, area_g = np.bincount(lp.ravel(), minlength=n_p + 1), np.bincount(lg.ravel(), minlength=n_g + 1)
        keep = area_p >= SETTINGS["min_area"]
        keep[0] = False
        F = keep[lp]
        hit_p, hit_g = np.bincount(lp[F & G[b]], minlength=n_p + 1), np.bincount(lg[G[b] & F], minlength=n_g + 1)
        filtered[b] = F
        stats.append(metrics.lesion_image_stats([P[b].sum(), F.sum(), G[b].sum(), n_p, keep.sum(), n_g, (keep & (hit_p >= 1)).sum(), (hit_g[1:] >= 1).sum(),
                                                 area_p[1:].max() if n_p else 0, area_g[1:].max() if n_g else 0, (F & G[b]).sum(), n_p - keep.sum()]))
    return stats, torch.from_numpy(filtered).cuda()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def device_ms(pred, lab, n=10):
    """The kernels alone by device events over the whole call, without the copy of the integers: the median of n."""
    out = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        kernels.lesion_score(pred, lab, 1, **SETTINGS)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out)


def bench(iters, inputs, sizes, batches):
    try:
        import scipy  # noqa: F401
        paths = (("fused", fused), ("literal", literal), ("scipy", host_scipy))
    except ImportError:
        paths = (("fused", fused), ("literal", literal))
        print("scipy is not importable: the host path is not measured")
    print("%-8s %-11s %3s | %10s %5s | %10s %5s | %10s %5s | %9s | %9s %7s | %7s %7s | %s" % (
        "input", "size", "B", "fused ms", "runs", "literal ms", "runs", "scipy ms", "runs", "device ms", "floor us", "x floor", "comp P", "comp G", "agreement"))
    for kind in inputs:
        for H, W in sizes:
            for B in batches:
                pred, lab = make(kind, B, H, W)
                run = []
                for n, fn in paths:                                    # a path that needs more than SKIP_S for one image is not run on sixteen
                    try:
                        one = timed(lambda: fn(pred[:1], lab[:1]))[0] if n != "fused" else 0.0
                    except RuntimeError as e:
                        if "no fixed point" not in str(e):             # anything else, a device error above all, ends the run
                            raise
                        print("%-8s %-11s %3d | %s not run: %s" % (kind, "%dx%d" % (H, W), B, n, e), flush=True)
                        continue
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
                same = ["%s %s" % (n, "equal" if outs[n][0] == outs["fused"][0] and torch.equal(outs[n][1], outs["fused"][1]) else "DIFFERS")
                        for n in outs if n != "fused"]
                floor_us = B * H * W * 10 / HBM_BYTES_PER_S * 1e6
                med = {n: statistics.median(times[n]) for n in times}
                dev = device_ms(pred, lab)
                cols = "".join(" %10.3f %5d |" % (med[n], len(times[n])) if n in med else " %10s %5s |" % ("-", "-") for n in ("fused", "literal", "scipy"))
                s0 = outs["fused"][0][0]
                print("%-8s %-11s %3d |%s %9.3f | %9.1f %7.1f | %7d %7d | %s" % (
                    kind, "%dx%d" % (H, W), B, cols, dev, floor_us, dev * 1e3 / floor_us, s0["pred_components"], s0["lesions"], ", ".join(same)), flush=True)


def kernels_only(n, inputs, sizes, batches):
    for kind in inputs:
        for H, W in sizes:
            for B in batches:
                pred, lab = make(kind, B, H, W)
                for _ in range(n):
                    kernels.lesion_score(pred, lab, 1, **SETTINGS)
                torch.cuda.synchronize()
                print("ran", kind, H, W, B, n, flush=True)


class _Stub(torch.nn.Module):
    def __init__(self, maps):
        super().__init__()
        self.maps = maps

    def forward(self, x):
        return (self.maps, self.maps, self.maps, self.maps)


def tester_cost(iters):
    """PranetTester.test() on a stub net (no backbone: the tail alone) over 8 batches of B images, keys off and on, alternating."""
    log = logging.getLogger("lesion_bench")
    log.addHandler(logging.NullHandler())
    log.propagate = False
    print("%-11s %3s %6s | %10s %10s | %s" % ("size", "B", "polyp", "off ms", "on ms", "cost of the keys per image, us"))
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
                    cfg.merge_from_list(["MODEL.NUM_CLASSES", 2, "OUTPUT_DIR", tempfile.mkdtemp(), "TEST.POLYP_METRICS", polyp, "TEST.LESION_METRICS", on,
                                         "TEST.MASK_MIN_AREA", 64 if on else 0])
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
    assert torch.cuda.is_available(), "lesion_bench needs the MI355X"
    sel = ((a.case,) if a.case else INPUTS, (tuple(int(v) for v in a.size.split("x")),) if a.size else SIZES, (a.batch,) if a.batch else BATCHES)
    if a.kernels:
        kernels_only(a.kernels, *sel)
    elif a.tester:
        tester_cost(a.iters)
    else:
        bench(a.iters, *sel)


if __name__ == "__main__":
    main()
