"""The definition of the boundary histograms (include/mi355seg.h, mi_boundary_score) restated in plain numpy and Python loops - row runs, then
the column walk - independent of the torch composition in host/metrics.py, plus the seeded inputs the boundary tests share."""
import numpy as np


def class_maps(pred, labels, K, ignore_index):
    """G and P as int64 arrays: a class in [0, K) or 255."""
    labels = np.asarray(labels).astype(np.int64)
    pred = np.asarray(pred).astype(np.int64)
    G = np.where((labels >= 0) & (labels < K), labels, 255)
    P = np.where(labels == ignore_index, 255, np.where((pred >= 0) & (pred < K), pred, 255))
    return G, P


def row_half_widths(L, D):
    """a(y, x) = min(D, the largest r with L(y, x-r .. x+r) inside the row and all equal to L(y, x)), from the runs of every row."""
    H, W = L.shape
    a = np.zeros((H, W), dtype=np.int64)
    for y in range(H):
        x = 0
        while x < W:
            end = x
            while end + 1 < W and L[y, end + 1] == L[y, x]:
                end += 1
            for i in range(x, end + 1):
                a[y, i] = min(D, i - x, end - i)
            x = end + 1
    return a


def survival(L, K, D):
    """e_L: radius r + 1 holds iff rows y - (r+1) and y + (r+1) exist, carry L(y, x) in column x, and the minimum of a over the rows
    y - (r+1) .. y + (r+1) of column x is >= r + 1.  0 where L has no class."""
    H, W = L.shape
    a = row_half_widths(L, D)
    e = np.zeros((H, W), dtype=np.int64)
    for y in range(H):
        for x in range(W):
            if not 0 <= L[y, x] < K:
                continue
            r, low = 0, a[y, x]
            while r < D:
                up, dn = y - (r + 1), y + (r + 1)
                if up < 0 or dn >= H or L[up, x] != L[y, x] or L[dn, x] != L[y, x]:
                    break
                low = min(low, a[up, x], a[dn, x])
                if low < r + 1:
                    break
                r += 1
            e[y, x] = r
    return e


def histograms(pred, labels, K, ignore_index, D):
    """int64 [5, K, D + 1]: what one call adds to hist."""
    G, P = class_maps(pred, labels, K, ignore_index)
    eG, eP = survival(G, K, D), survival(P, K, D)
    hist = np.zeros((5, K, D + 1), dtype=np.int64)
    H, W = G.shape
    for y in range(H):
        for x in range(W):
            g, p = G[y, x], P[y, x]
            if g < K:
                hist[0, g, eG[y, x]] += 1
            if p < K:
                hist[1, p, eP[y, x]] += 1
            if g < K and g == p:
                hist[2, g, max(eG[y, x], eP[y, x])] += 1
                hist[3, g, eG[y, x]] += 1
            if p < K and g < K:
                hist[4, p, eG[y, x]] += 1
    return hist


def block_labels(H, W, K, seed, block=(9, 13), holes=0.03, ignore_index=255, stray=0.0):
    """A block-structured int64 label map: blocks of random sizes around `block` with random classes, `holes` of the pixels set to ignore_index
    singly and in one rectangle, and `stray` of them set to values outside [0, K) that are not the ignore index (-1, K, 254)."""
    rng = np.random.RandomState(seed)
    lab = np.zeros((H, W), dtype=np.int64)
    y = 0
    while y < H:
        bh = int(rng.randint(1, 2 * block[0]))
        x = 0
        while x < W:
            bw = int(rng.randint(1, 2 * block[1]))
            lab[y:y + bh, x:x + bw] = rng.randint(0, K)
            x += bw
        y += bh
    if holes > 0:
        lab[rng.rand(H, W) < holes] = ignore_index
        y0, x0 = int(rng.randint(0, H)), int(rng.randint(0, W))
        lab[y0:y0 + max(1, H // 6), x0:x0 + max(1, W // 5)] = ignore_index
    if stray > 0:
        sel = rng.rand(H, W) < stray
        lab[sel] = rng.choice(np.array([-1, K, 254], dtype=np.int64), size=int(sel.sum()))
    return lab


def shifted_prediction(labels, K, seed, shift=(2, 3), noise=0.02, beyond=0.0):
    """The uint8 prediction the tests pair with `labels`: the label map moved by `shift` (so that the two erosion counts of a pixel differ), values
    outside [0, K) replaced by random classes, `noise` of the pixels redrawn, `beyond` of them set to values >= K (K, 200, 255)."""
    rng = np.random.RandomState(seed)
    pred = np.roll(np.asarray(labels), shift, axis=(0, 1)).copy()
    bad = (pred < 0) | (pred >= K)
    pred[bad] = rng.randint(0, K, size=int(bad.sum()))
    sel = rng.rand(*pred.shape) < noise
    pred[sel] = rng.randint(0, K, size=int(sel.sum()))
    if beyond > 0:
        sel = rng.rand(*pred.shape) < beyond
        pred[sel] = rng.choice(np.array([min(K, 255), 200, 255]), size=int(sel.sum()))
    return pred.astype(np.uint8)
