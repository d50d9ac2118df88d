"""A literal float64 restatement of the polyp evaluation (TEST.POLYP_METRICS) on materialised arrays: the map PranetTester.predict thresholds and the
metrics of the published evaluation code (Dice / IoU / F-beta per threshold, E-measure on the actual alignment matrix, S-measure on real quadrant
slices with np.std(ddof=1), MAE).  Shares no code with host/metrics.py, which derives the same numbers from a histogram and moment sums.
Two departures from the published code, both where it yields NaN: a quadrant of fewer than 2 pixels contributes 0 to the S-measure, and the
standard deviation of fewer than 2 values is 0.
`counted` states, in numpy, what the kernel mi_polyp_score returns for a given fp32 map and labels (the staging of tests/test_gpu_classwise.py)."""
import numpy as np

EPS = 2.220446049250313e-16


# ------------------------------------------------------------------------------------------------ the map
def _axis(n_in, n_out):
    """F.interpolate(mode='bilinear', align_corners=False): source index max(scale (dst + 0.5) - 0.5, 0) in float64, the two taps and lambda."""
    src = np.maximum((n_in / n_out) * (np.arange(n_out, dtype=np.float64) + 0.5) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, src - i0


def reference_logits(low, size):
    low = np.asarray(low, dtype=np.float64)
    y0, y1, ly = _axis(low.shape[1], size[0])
    x0, x1, lx = _axis(low.shape[2], size[1])
    ly, lx = ly[None, :, None], lx[None, None, :]
    top = low[:, y0][:, :, x0] * (1 - lx) + low[:, y0][:, :, x1] * lx
    bot = low[:, y1][:, :, x0] * (1 - lx) + low[:, y1][:, :, x1] * lx
    return top * (1 - ly) + bot * ly


def reference_map(low, size):
    """low [B,h,w] -> float64 [B,H,W]: bilinear, sigmoid, min-max over the whole batch (pranet_tester.py:37-43)."""
    p = 1.0 / (1.0 + np.exp(-reference_logits(low, size)))
    return (p - p.min()) / (p.max() - p.min() + 1e-8)


def quantise(p):
    """q = int(float32(p) * float32(255)), truncated."""
    return (np.asarray(p).astype(np.float32) * np.float32(255)).astype(np.int64)


# ------------------------------------------------------------------------------------------------ the metrics
def _ratio(num, den, both_empty):
    if den == 0:
        return 1.0 if both_empty else 0.0
    return num / den


def _object(x):
    mean = x.mean()
    std = np.std(x, ddof=1) if x.size > 1 else 0.0
    return 2.0 * mean / (mean ** 2 + 1.0 + std + EPS)


def _ssim(p, g):
    n = p.size
    if n < 2:
        return 0.0
    x, y = p.mean(), g.mean()
    var_p = ((p - x) ** 2).sum() / (n - 1)
    var_g = ((g - y) ** 2).sum() / (n - 1)
    cov = ((p - x) * (g - y)).sum() / (n - 1)
    a = 4 * x * y * cov
    b = (x ** 2 + y ** 2) * (var_p + var_g)
    if a != 0:
        return a / (b + EPS)
    return 1.0 if b == 0 else 0.0


def s_measure(p, g):
    H, W = g.shape
    y = g.mean()
    if y == 0:
        return 1.0 - p.mean()
    if y == 1:
        return p.mean()
    s_obj = y * _object(p[g == 1]) + (1 - y) * _object(1.0 - p[g == 0])
    rows, cols = np.nonzero(g)
    cx, cy = int(np.rint(cols.sum() / g.sum())) + 1, int(np.rint(rows.sum() / g.sum())) + 1
    N = H * W
    w1, w2, w3 = cx * cy / N, cy * (W - cx) / N, (H - cy) * cx / N
    s_reg = (w1 * _ssim(p[:cy, :cx], g[:cy, :cx]) + w2 * _ssim(p[:cy, cx:], g[:cy, cx:]) + w3 * _ssim(p[cy:, :cx], g[cy:, :cx])
             + (1 - w1 - w2 - w3) * _ssim(p[cy:, cx:], g[cy:, cx:]))
    return max(0.0, 0.5 * s_obj + 0.5 * s_reg)


def e_measure(binary, g):
    N = g.size
    G = g.sum()
    if G == 0:
        enhanced = 1.0 - binary
    elif G == N:
        enhanced = binary.copy()
    else:
        db, dg = binary - binary.mean(), g - g.mean()
        align = 2 * db * dg / (db * db + dg * dg + EPS)
        enhanced = (align + 1) ** 2 / 4
    return enhanced.sum() / (N - 1 + EPS)


def reference_metrics(p, g):
    """p float64 [H,W] in [0,1], g [H,W] in {0,1} -> {"dice", "iou", "f", "e": [256] curves, "S", "MAE"}, binarising per threshold in a loop."""
    p = np.asarray(p, dtype=np.float64)
    g = np.asarray(g).astype(np.float64)
    q = quantise(p)
    G = g.sum()
    out = {k: np.zeros(256) for k in ("dice", "iou", "f", "e")}
    for t in range(256):
        binary = (q >= t).astype(np.float64)
        tp, fp = (binary * g).sum(), (binary * (1 - g)).sum()
        empty = binary.sum() == 0 and G == 0
        out["dice"][t] = _ratio(2 * tp, tp + fp + G, empty)
        out["iou"][t] = _ratio(tp, fp + G, empty)
        prec, rec = _ratio(tp, tp + fp, empty), _ratio(tp, G, empty)
        out["f"][t] = _ratio(1.3 * prec * rec, 0.3 * prec + rec, empty)
        out["e"][t] = e_measure(binary, g)
    out["S"] = float(s_measure(p, g))
    out["MAE"] = float(np.abs(p - g).mean())
    return out


def aggregate(per_image):
    """The dataset numbers from a list of reference_metrics results: curves averaged over images, then mean / max over the thresholds."""
    c = {k: np.mean([r[k] for r in per_image], axis=0) for k in ("dice", "iou", "f", "e")}
    return {"mDice": float(c["dice"].mean()), "mIoU": float(c["iou"].mean()), "meanF": float(c["f"].mean()), "maxF": float(c["f"].max()),
            "S": float(np.mean([r["S"] for r in per_image])), "meanE": float(c["e"].mean()), "maxE": float(c["e"].max()),
            "MAE": float(np.mean([r["MAE"] for r in per_image])), "images": len(per_image)}, c


# ------------------------------------------------------------------------------------------------ what the kernel counts, in numpy
def counted(p, labels):
    """For one image: p [H,W] (the fp32 map, or any map), labels int [H,W] -> (hist int64 [2,256], sums float64 [24], counts int64 [4], pred uint8)
    in mi_polyp_score's layout, the sums in float64 from the given values."""
    p32 = np.asarray(p).astype(np.float32)
    labels = np.asarray(labels)
    H, W = labels.shape
    g = labels == 1
    q = quantise(p32)
    hist = np.stack([np.bincount(q[~g], minlength=256), np.bincount(q[g], minlength=256)]).astype(np.int64)
    rows, cols = np.nonzero(g)
    G = int(g.sum())
    counts = np.array([G, cols.sum(), rows.sum(), ((labels != 0) & (labels != 1)).sum()], dtype=np.int64)
    cx, cy = (int(round(int(cols.sum()) / G)) + 1, int(round(int(rows.sum()) / G)) + 1) if G else (0, 0)
    pd = p32.astype(np.float64)
    sums = np.zeros(24)
    for i, (ys, xs) in enumerate(((slice(0, cy), slice(0, cx)), (slice(0, cy), slice(cx, W)), (slice(cy, H), slice(0, cx)), (slice(cy, H), slice(cx, W)))):
        a, b = pd[ys, xs], g[ys, xs]
        sums[5 * i:5 * i + 5] = [a.sum(), (a * a).sum(), a[b].sum(), (a[b] * a[b]).sum(), b.sum()]
    sums[20], sums[21] = cx, cy
    pred = (p32 > np.float32(1) - p32).astype(np.uint8)
    return hist, sums, counts, pred
