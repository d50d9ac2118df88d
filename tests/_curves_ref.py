"""A numpy restatement of the two histograms of TEST.CURVES (include/mi355seg.h, mi_upsample_curves) with explicit loops over the classes,
independent of the torch code in host/metrics.py: what test_host_curves.py holds literal_curves against and test_gpu_curves.py the kernels."""
import numpy as np

BINS = 256
FIXED = 1 << 24


def curves_ref(probs, label, K, ece_bins):
    """probs [K,H,W] fp32, label [H,W] integers -> (pr int64 [K,256,2], cal int64 [ece_bins,3])."""
    probs = np.asarray(probs, dtype=np.float32)
    label = np.asarray(label).astype(np.int64)
    assert probs.shape == (K,) + label.shape
    M = int(ece_bins)
    counted = (label >= 0) & (label < K)
    pr = np.zeros((K, BINS, 2), dtype=np.int64)
    for k in range(K):
        scaled = probs[k] * np.float32(BINS)                                   # fp32 product: exact (a power of two)
        b = np.minimum(BINS - 1, np.maximum(0, np.trunc(scaled).astype(np.int64)))
        for side in (0, 1):
            sel = counted & ((label == k) == bool(side))
            pr[k, :, side] = np.bincount(b[sel], minlength=BINS)
    cal = np.zeros((M, 3), dtype=np.int64)
    conf = probs[0].copy()
    pred = np.zeros(label.shape, dtype=np.int64)
    for k in range(1, K):                                                      # strict: the lowest index among equal maxima stays
        better = probs[k] > conf
        conf[better] = probs[k][better]
        pred[better] = k
    m = np.minimum(M - 1, np.maximum(0, np.trunc(conf * np.float32(M)).astype(np.int64)))
    fixed = np.trunc(conf.astype(np.float64) * FIXED).astype(np.int64)         # a power-of-two scale: exact in either precision
    for j in range(M):
        sel = counted & (m == j)
        cal[j, 0] = int(sel.sum())
        cal[j, 1] = int((sel & (pred == label)).sum())
        cal[j, 2] = int(fixed[sel].sum())
    return pr, cal
