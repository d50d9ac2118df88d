"""The boundary loss's two kernels on one MI355X: the signed distance map (mi_signed_distance) against the host path a dataset worker would run, and
the fused Tversky + BCE head with and without the boundary term, alternating in one process.

  device   kernels.signed_distance on the mask where it lives (a memset and two launches, nothing read back)
  host     the mask copied to the host, scipy.ndimage.distance_transform_edt twice per image through the published line
           edt(~G) * ~G - (edt(G) - 1) * G, the float32 map copied back
  head     kernels.upsample_tversky_bce on PraNet's three head shapes (B x 11 / 22 / 44 squared -> 352 squared), plain and with phi

Masks are 16 x 352 x 352 (PraNet's training batch) and 1 x 1072 x 1920 (the largest Kvasir pictures); `compact` = one ellipse of about a sixth of
the picture, `speckle` = compact with 3 % of the pixels flipped (the inputs of tools/surface_bench.py).  A figure is the median wall time of one call,
the clock read after a device synchronise; the device path and the head are timed over --reps back-to-back calls between two synchronises.  The
byte floor of the map is the mask read and phi written once (8 bytes per pixel) over 4 TB/s.  --kernels N runs the device path N times per case and
nothing else, for a `rocprofv3 --kernel-trace --stats` run (the two kernels' own times).

    python tools/sdf_bench.py [--iters 10] [--reps 20] [--kernels N] [--case compact] [--shape 16x352x352]
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

SHAPES = ((16, 352, 352), (1, 1072, 1920))
INPUTS = ("compact", "speckle")
HBM_BYTES_PER_S = 4e12


def make(kind, B, H, W):
    """float32 {0, 1} [B,H,W] on the GPU; image b is shifted by b pixels so that the images of a batch differ."""
    g = np.random.RandomState(17)
    yy, xx = np.mgrid[0:H, 0:W]
    t = (((yy - 0.52 * H) / (0.20 * H)) ** 2 + ((xx - 0.48 * W) / (0.23 * W)) ** 2) < 1
    if kind == "speckle":
        t = t ^ (g.rand(H, W) < 0.03)
    return torch.from_numpy(np.stack([np.roll(t, b, 0) for b in range(B)]).astype(np.float32)).cuda()


def host_path(mask):
    from scipy import ndimage as ndi
    G = mask.cpu().numpy() >= 0.5
    out = np.zeros(G.shape, np.float32)
    for b in range(G.shape[0]):
        if G[b].any() and not G[b].all():
            out[b] = ndi.distance_transform_edt(~G[b]) * ~G[b] - (ndi.distance_transform_edt(G[b]) - 1) * G[b]
    return torch.from_numpy(out).cuda()


def timed(fn, reps=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps, out


def distance_maps(iters, reps):
    try:
        import scipy  # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False
        print("scipy is not importable: the host path is not measured")
    print("%-8s %-14s | %10s | %10s %5s | %9s %8s | %s" % ("input", "shape", "device ms", "host ms", "runs", "floor us", "x floor", "equal bits"))
    for kind in INPUTS:
        for B, H, W in SHAPES:
            mask = make(kind, B, H, W)
            dev = timed(lambda: kernels.signed_distance(mask))[1]
            same = "-"
            if have_scipy:
                same = str(bool(torch.equal(dev.view(torch.int32), timed(lambda: host_path(mask))[1].view(torch.int32))))
            t_dev, t_host = [], []
            for _ in range(iters):                                     # alternating
                t_dev.append(timed(lambda: kernels.signed_distance(mask), reps)[0])
                if have_scipy and (len(t_host) < 2 or sum(t_host) < 4e3):
                    t_host.append(timed(lambda: host_path(mask))[0])
            floor_us = B * H * W * 8 / HBM_BYTES_PER_S * 1e6
            d = statistics.median(t_dev)
            print("%-8s %-14s | %10.4f | %10.3f %5d | %9.2f %8.1f | %s" % (kind, "%dx%dx%d" % (B, H, W), d, statistics.median(t_host) if t_host else float("nan"),
                                                                          len(t_host), floor_us, d * 1e3 / floor_us, same), flush=True)


def heads(iters, reps, B=16, S=352):
    mask = make("compact", B, S, S)
    phi = kernels.signed_distance(mask)
    print("%-22s | %10s %10s | %s" % ("head (forward + dlow)", "plain ms", "with phi ms", "difference us"))
    for f in (32, 16, 8):
        low = torch.from_numpy(np.random.RandomState(f).randn(B, S // f, S // f).astype(np.float32)).cuda()
        plain = lambda: kernels.upsample_tversky_bce(low, mask)
        sdf = lambda: kernels.upsample_tversky_bce(low, mask, phi=phi, w_boundary=0.01)
        timed(plain), timed(sdf)
        t = {"plain": [], "sdf": []}
        for _ in range(iters):
            t["plain"].append(timed(plain, reps)[0])
            t["sdf"].append(timed(sdf, reps)[0])
        a, b = statistics.median(t["plain"]), statistics.median(t["sdf"])
        print("%-22s | %10.4f %10.4f | %.1f" % ("%dx%dx%d -> %d" % (B, S // f, S // f, S), a, b, (b - a) * 1e3), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kernels", type=int, default=0)
    ap.add_argument("--case", choices=INPUTS, default=None, help="with --kernels: one input only")
    ap.add_argument("--shape", default=None, help="with --kernels: one shape only, BxHxW")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "sdf_bench needs the MI355X"
    if a.kernels:
        for kind in ((a.case,) if a.case else INPUTS):
            for B, H, W in ((tuple(int(v) for v in a.shape.split("x")),) if a.shape else SHAPES):
                mask = make(kind, B, H, W)
                for _ in range(a.kernels):
                    kernels.signed_distance(mask)
                torch.cuda.synchronize()
                print("ran", kind, B, H, W, a.kernels, flush=True)
        return
    distance_maps(a.iters, a.reps)
    heads(a.iters, a.reps)


if __name__ == "__main__":
    main()
