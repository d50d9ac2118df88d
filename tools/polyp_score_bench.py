"""The polyp evaluation tail (TEST.POLYP_METRICS): the fused kernels (mi_polyp_score) against the literal composition from torch ops, alternating in
one process on one MI355X.  Maps are 352 x 352 (PraNet's res2), labels 352 x 352 and 1072 x 1920 (the largest Kvasir pictures), B = 1 and 16.

  fused    kernels.polyp_score (init, scan, score, finalize: four small launches; the mask included), then ONE device-to-host copy each of the
           histogram, the sums and the counts
  literal  what one would write without it: gk.gresize -> sigmoid -> batch min-max -> the mask -> quantise -> torch.bincount -> the label
           centroid (a host sync per image) -> the per-quadrant moment sums from slices, then the same device-to-host copies

Three inputs: `spread` = the res2 map of an untrained PraNet on synthetic polyp images (its logits spread, but a few outliers set the batch's
min-max, so most normalised pixels still fall in a handful of bins: the share is printed), `uniform` = independent N(0, 2) logits (every bin
occupied), `saturated` = logits of +/-12 following the ground truth except in a band (what a trained net produces: almost every pixel in bin 0
or bins 254 / 255, the worst case for histogram contention).  A figure is the wall time of one call, the clock read after a device synchronise;
--kernels N runs the fused tail N times per case and nothing else, for a `rocprofv3 --kernel-trace --stats` run (the kernels' own times).

    python tools/polyp_score_bench.py [--iters 20] [--kernels N]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rnd_semantic_segmentation_amd import gk, kernels  # noqa: E402
from rnd_semantic_segmentation_amd.host import pranet, synth  # noqa: E402

MAP = 352
LABELS = ((352, 352), (1072, 1920))
BATCHES = (1, 16)
REGIMES = ("spread", "uniform", "saturated")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def fused(low, y):
    r = kernels.polyp_score(low, y, want_prob=False, want_pred=True)
    return r.hist.cpu().numpy(), r.sums.cpu().numpy(), r.counts.cpu().numpy(), r.pred


def literal(low, y):
    B, H, W = y.shape
    p = gk.gresize(low.unsqueeze(3).contiguous(), (H, W), False).squeeze(3).sigmoid()
    p = (p - p.min()) / (p.max() - p.min() + 1e-8)
    pred = (p > 1 - p).to(torch.uint8)
    g = y == 1
    q = (p * 255.0).long()
    image = torch.arange(B, device=y.device).view(B, 1, 1)
    hist = torch.bincount((image * 512 + g.long() * 256 + q).flatten(), minlength=B * 512).reshape(B, 2, 256)
    cols = torch.arange(W, device=y.device).view(1, 1, W)
    rows = torch.arange(H, device=y.device).view(1, H, 1)
    counts = torch.stack([g.sum((1, 2)), (g * cols).sum((1, 2)), (g * rows).sum((1, 2)), ((y != 0) & (y != 1)).sum((1, 2))], 1)
    counts_host = counts.cpu().numpy()
    pd = p.double()
    sums = torch.zeros(B, kernels.POLYP_SUMS, dtype=torch.float64, device=y.device)
    for b in range(B):
        G = int(counts_host[b, 0])
        cx, cy = (int(round(int(counts_host[b, 1]) / G)) + 1, int(round(int(counts_host[b, 2]) / G)) + 1) if G else (0, 0)
        for i, (ys, xs) in enumerate(((slice(0, cy), slice(0, cx)), (slice(0, cy), slice(cx, W)), (slice(cy, H), slice(0, cx)), (slice(cy, H), slice(cx, W)))):
            a, m = pd[b, ys, xs], g[b, ys, xs]
            am = a * m
            sums[b, 5 * i:5 * i + 5] = torch.stack([a.sum(), (a * a).sum(), am.sum(), (am * a).sum(), m.sum().double()])
        sums[b, 20], sums[b, 21] = cx, cy
    return hist.cpu().numpy(), sums.cpu().numpy(), counts_host, pred


def inputs(B, H, W, regime):
    img, mask = synth.synth_polyp(B, MAP, MAP, seed=17)
    mask_t = torch.from_numpy(mask).cuda()
    y = torch.nn.functional.interpolate(mask_t, size=(H, W), mode="nearest").reshape(B, H, W).long().contiguous()
    if regime == "spread":
        torch.manual_seed(7)
        net = pranet.PraNet().cuda().eval()
        net.set_precision("bf16")
        with torch.no_grad():
            low = net(torch.from_numpy(img).cuda())[3].float().reshape(B, MAP, MAP).contiguous()
        del net
    elif regime == "uniform":
        g = torch.Generator(device="cpu").manual_seed(6)
        low = (2.0 * torch.randn(B, MAP, MAP, generator=g)).cuda().contiguous()
    else:
        sign = mask_t.reshape(B, MAP, MAP) * 2 - 1
        sign[:, :, :MAP // 6] *= -1
        g = torch.Generator(device="cpu").manual_seed(5)
        low = (sign * (12.0 + torch.randn(B, MAP, MAP, generator=g).cuda())).contiguous()
    return low, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--kernels", type=int, default=0)
    args = ap.parse_args()
    for H, W in LABELS:
        for B in BATCHES:
            for regime in REGIMES:
                low, y = inputs(B, H, W, regime)
                if args.kernels:
                    for _ in range(args.kernels):
                        kernels.polyp_score(low, y, want_prob=False, want_pred=True)
                    torch.cuda.synchronize()
                    continue
                for _ in range(2):                               # warm-up of every shape of both paths
                    f, l = fused(low, y), literal(low, y)
                moved = int(np.abs(f[0] - l[0]).sum()) // 2          # pixels whose bin differs: gresize and the kernel round the lerp differently
                ends = float(f[0][:, :, [0, 254, 255]].sum()) / f[0].sum()
                same = np.array_equal(f[2], l[2]) and np.array_equal(f[1][:, 20:22], l[1][:, 20:22])
                tf, tl = [], []
                for _ in range(args.iters):                      # alternating: drift of the clocks hits both alike
                    tf.append(timed(lambda: fused(low, y))[0])
                    tl.append(timed(lambda: literal(low, y))[0])
                print("labels %dx%d, B=%d, %s (%.0f%% of the pixels in bins 0 / 254 / 255; counts and split points equal: %s; %d of %d pixels in "
                      "another bin; %d alternating iterations):" % (H, W, B, regime, 100 * ends, same, moved, B * H * W, args.iters))
                print("  fused median %8.3f ms (min %.3f, max %.3f)   literal median %8.3f ms (min %.3f, max %.3f)   literal / fused %.2f"
                      % (statistics.median(tf), min(tf), max(tf), statistics.median(tl), min(tl), max(tl), statistics.median(tl) / statistics.median(tf)))


if __name__ == "__main__":
    main()
