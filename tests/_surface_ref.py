"""Brute-force numpy restatement of the surface-distance definitions of include/mi355seg.h (mi_surface_score): surfaces from padded shifts,
integer d2 by broadcasting over the two coordinate lists, numpy's percentile.  Shares nothing with the kernel or with host/metrics.py.  Also the
input cases of tests/test_host_surface.py and tests/test_gpu_surface.py."""
import math

import numpy as np

INTS = 27
MAX_TOL = 8


def surface(mask):
    """M & ~binary_erosion(M, cross, border_value=0): foreground pixels with a four-neighbour outside M; outside the image is outside M."""
    m = np.asarray(mask, dtype=bool)
    p = np.pad(m, 1, constant_values=False)
    inner = p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]
    return m & ~inner


def directed_d2(src, dst, chunk=2048):
    """For every point of src [n, 2] the smallest squared distance to a point of dst [m, 2]: int64 [n], in the order of src."""
    out = np.empty(len(src), np.int64)
    for i in range(0, len(src), chunk):
        d = src[i:i + chunk, None, :].astype(np.int64) - dst[None, :, :].astype(np.int64)
        out[i:i + chunk] = (d * d).sum(-1).min(1)
    return out


def tol2(tolerances):
    return [int(math.floor(float(t) * float(t))) for t in tolerances]


def reference(pred, label, cls=1, q=95, tolerances=()):
    """One image.  Returns (ints int64 [27] as mi_surface_score lays them out, (d2 from S(P), d2 from S(G)) or None, metrics dict).  The metrics:
    HD, HDq, ASSD (None where undefined), NSD (list per tolerance), defined."""
    P, G = np.asarray(pred) == cls, np.asarray(label) == cls
    sp, sg = surface(P), surface(G)
    a, b = np.argwhere(sp), np.argwhere(sg)
    ints = np.zeros(INTS, np.int64)
    ints[:4] = P.sum(), G.sum(), len(a), len(b)
    n = len(a) + len(b)
    t2 = tol2(tolerances)
    if n == 0:
        ints[10] = 1
        return ints, None, {"HD": 0.0, "HDq": 0.0, "ASSD": 0.0, "NSD": [1.0] * len(t2), "defined": True}
    if len(a) == 0 or len(b) == 0:
        return ints, None, {"HD": None, "HDq": None, "ASSD": None, "NSD": [0.0] * len(t2), "defined": False}
    dp, dg = directed_d2(a, b), directed_d2(b, a)
    both = np.sort(np.concatenate([dp, dg]))
    fl, rem = divmod(q * (n - 1), 100)
    ints[4:11] = dp.max(), dg.max(), both[fl], both[min(fl + 1, n - 1)], fl, rem, 1
    for t, v in enumerate(t2):
        ints[11 + 2 * t], ints[12 + 2 * t] = (dp <= v).sum(), (dg <= v).sum()
    fp, fg = np.sqrt(dp.astype(np.float64)), np.sqrt(dg.astype(np.float64))
    metrics = {"HD": float(max(fp.max(), fg.max())), "HDq": float(np.percentile(np.concatenate([fp, fg]), q)),
               "ASSD": float((fp.mean() + fg.mean()) / 2), "NSD": [float(((dp <= v).sum() + (dg <= v).sum()) / n) for v in t2], "defined": True}
    return ints, (dp, dg), metrics


def sums(d2):
    """The two directed sums of sqrt(d2) in float64 (math.fsum: correctly rounded), (0, 0) without distances."""
    if d2 is None:
        return 0.0, 0.0
    return tuple(math.fsum(np.sqrt(d.astype(np.float64))) for d in d2)


# ------------------------------------------------------------------------------------------------ the cases
def rect(H, W, y0, y1, x0, x1):
    m = np.zeros((H, W), np.int64)
    m[y0:y1, x0:x1] = 1
    return m


def ellipse(H, W, cy, cx, ry, rx):
    yy, xx = np.mgrid[0:H, 0:W]
    return ((((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2) < 1).astype(np.int64)


def speckle(m, share, seed):
    g = np.random.RandomState(seed)
    return np.where(g.rand(*m.shape) < share, 1 - m, m)


def ring_count(n):
    """A one-pixel-wide horizontal line of n pixels in a 5 x (n + 2) image: exactly n surface pixels."""
    return rect(5, n + 2, 2, 3, 1, n + 1)


def cases():
    """name -> (pred uint8 [H, W], label int64 [H, W]); every mask of every case is non-empty (the empty ones live in the batch cases)."""
    out = {}

    def add(name, p, g):
        out[name] = (p.astype(np.uint8), g.astype(np.int64))

    add("1x1", np.ones((1, 1)), np.ones((1, 1)))
    p, g = np.zeros((1, 70)), np.zeros((1, 70))
    p[0, 2:9], p[0, 66] = 1, 1
    g[0, 60:69], g[0, 0] = 1, 1
    add("row_1x70", p, g)                                               # crosses a wave boundary, no vertical extent
    add("col_70x1", p.T.copy(), g.T.copy())
    p, g = np.zeros((37, 45)), np.zeros((37, 45))
    p[0, 0], g[36, 44] = 1, 1
    add("corners_37x45", p, g)                                          # d2 = 36^2 + 44^2, every other column without a site, n = 2
    add("full_vs_rect_33x64", np.ones((33, 64)), rect(33, 64, 10, 20, 20, 50))      # the surface of the full mask is the image frame
    p, g = np.zeros((33, 64)), np.zeros((33, 64))
    p[5, 3:60], p[5:30, 31] = 1, 1
    g[20, 0:64], g[2:19, 10] = 1, 1
    add("lines_33x64", p, g)                                            # one pixel wide, no crossing: every pixel is surface
    add("speckle_37x45", speckle(rect(37, 45, 8, 30, 10, 36), 0.03, 1), speckle(rect(37, 45, 10, 33, 7, 33), 0.03, 2))
    add("speckle_33x64", speckle(rect(33, 64, 4, 28, 9, 55), 0.03, 3), speckle(rect(33, 64, 6, 30, 12, 60), 0.03, 4))
    add("far_blobs_200x517", ellipse(200, 517, 60, 70, 40, 50), ellipse(200, 517, 130, 440, 50, 60))
    add("n21", ring_count(10), np.roll(ring_count(11)[:, :12], 1, axis=0))          # 10 + 11 surface pixels: 95 * 20 / 100 = 19 exactly
    add("n41", ring_count(20), np.roll(ring_count(21)[:, :22], 1, axis=0))          # 95 * 40 / 100 = 38 exactly
    add("n23", ring_count(11), np.roll(ring_count(12)[:, :13], 1, axis=0))          # 95 * 22 / 100 = 20.9
    return out


def multi_class_map(H, W, seed):
    """A map with the values 0..4 in blocks plus noise, for cls = 3."""
    g = np.random.RandomState(seed)
    m = (np.add.outer(np.arange(H) // 7, np.arange(W) // 9) % 5).astype(np.int64)
    noise = g.rand(H, W) < 0.05
    m[noise] = g.randint(0, 5, int(noise.sum()))
    return m
