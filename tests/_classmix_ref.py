"""numpy restatement of the ClassMix kernels' integer side (csrc/classmix.hip): the class bit sets, the selection rule, the mixing given the
pseudo-labels, the counts; and the exact EMA with its rounding bound.  The pseudo-labels themselves are not restated: their oracle is
kernels.upsample_predict_score, which has its own parity tests."""
import numpy as np


def present_bits(labels, K):
    """labels [B,H,W] int64 -> uint32 [B]: bit c set iff class c in [0, K) occurs in image b; everything else sets nothing."""
    out = np.zeros(labels.shape[0], dtype=np.uint32)
    for b, lab in enumerate(labels):
        for c in np.unique(lab):
            if 0 <= c < K:
                out[b] |= np.uint32(1) << np.uint32(c)
    return out


def chosen_classes(present, priority, K):
    """The ceil(n/2) classes of `present` (bits below K) with the smallest priority[c], n their number, as a python int bit set."""
    classes = [c for c in range(K) if (int(present) >> c) & 1]
    take = (len(classes) + 1) // 2
    picked = sorted(classes, key=lambda c: int(priority[c]))[:take]
    return sum(1 << c for c in picked)


def classmix(src_img, tgt_img, src_lab, pseudo, present, priority, K, ignore_index):
    """pseudo [B,H,W] uint8 with 255 = below the threshold (upsample_predict_score's pseudo output per image).
    Returns (mix_img, mix_lab, mask uint8, counts int64 [B,2])."""
    B = src_lab.shape[0]
    mask = np.zeros(src_lab.shape, dtype=bool)
    for b in range(B):
        ch = chosen_classes(present[b], priority[b], K)
        lab = src_lab[b]
        ok = (lab >= 0) & (lab < K)
        sel = np.zeros(lab.shape, dtype=bool)
        sel[ok] = ((ch >> lab[ok]) & 1).astype(bool)
        mask[b] = sel
    ps = pseudo.astype(np.int64)
    kept = pseudo != 255
    ps[~kept] = ignore_index
    mix_img = np.where(mask[:, None], src_img, tgt_img)
    mix_lab = np.where(mask, src_lab, ps)
    counts = np.stack([mask.reshape(B, -1).sum(1), (kept & ~mask).reshape(B, -1).sum(1)], 1).astype(np.int64)
    return mix_img, mix_lab, mask.astype(np.uint8), counts


def ema_exact(teacher, student, a):
    """(exact float64 result, bound) of teacher = a * teacher + b * student with the fp32 a and the fp32 b = 1.0f - a:
    |out - exact| <= 3 * 2**-24 * (|a t| + |b s|), two rounded products and one rounded sum."""
    a32 = np.float32(a)
    b32 = np.float32(1.0) - a32
    at = np.float64(a32) * teacher.astype(np.float64)
    bs = np.float64(b32) * student.astype(np.float64)
    return at + bs, 3.0 * 2.0 ** -24 * (np.abs(at) + np.abs(bs))
