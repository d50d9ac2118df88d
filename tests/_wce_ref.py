"""Float64 restatement of torch.nn.CrossEntropyLoss(weight=, ignore_index=, label_smoothing=) on bilinearly upsampled logits, with its gradient
written out, a second function that takes both from F.cross_entropy by autograd, and the case table of tests/test_host_wce.py / tests/test_gpu_wce.py.

    z = bilinear(low), p = softmax(z), m = label valid (not ignore_index, inside [0, K)), y = label, s = label_smoothing, Wsum = sum_c w_c
    S       = sum_valid w_y
    loss    = [ (1-s) sum_valid w_y (-log p_y) + s/K sum_valid sum_c w_c (-log p_c) ] / S
    dl/dz_k = m [ (1-s) w_y (p_k - [k==y]) + s/K (p_k Wsum - w_k) ] / S
    d loss / d low = the transposed bilinear of d loss / d z
"""
import collections

import numpy as np
import torch
import torch.nn.functional as F

from rnd_semantic_segmentation_amd.host import synth

WceRef = collections.namedtuple("WceRef", "loss S bad dlow")          # dlow [B,h,w,K] (the kernels' layout)


def _low64(low):
    """low [B,h,w,K] (NHWC, any float dtype) -> [B,K,h,w] float64 leaf"""
    return torch.as_tensor(np.asarray(low)).double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)


def wce_ref(low, labels, weights=None, smoothing=0.0, align_corners=True, ignore_index=255):
    """low [B,h,w,K], labels [B,H,W] int64, weights [K] or None -> WceRef in float64.  Labels outside [0, K) that are not ignore_index are left out
    and counted in `bad`."""
    x = _low64(low)
    lab = torch.as_tensor(np.asarray(labels)).long()
    K = x.shape[1]
    w = torch.ones(K, dtype=torch.float64) if weights is None else torch.as_tensor(np.asarray(weights)).double()
    z = F.interpolate(x, size=tuple(lab.shape[-2:]), mode="bilinear", align_corners=align_corners)
    zd = z.detach()
    lp = zd - zd.max(1, keepdim=True).values
    lp = lp - torch.log(torch.exp(lp).sum(1, keepdim=True))          # (z - max) - log(sum exp)
    p = torch.exp(lp)
    valid = (lab != ignore_index) & (lab >= 0) & (lab < K)
    bad = int(((lab != ignore_index) & ~valid).sum())
    y = torch.where(valid, lab, torch.zeros_like(lab))
    m = valid.double().unsqueeze(1)
    onehot = F.one_hot(y, K).permute(0, 3, 1, 2).double()
    wy = (w[y] * valid.double()).unsqueeze(1)                        # [B,1,H,W]
    wv = w.view(1, K, 1, 1)
    s = float(smoothing)
    S = wy.sum()
    hard = (wy * -(lp * onehot).sum(1, keepdim=True)).sum()
    soft = (m * -(lp * wv).sum(1, keepdim=True)).sum()
    loss = ((1.0 - s) * hard + s / K * soft) / S
    dz = m * ((1.0 - s) * wy * (p - onehot) + s / K * (p * w.sum() - wv)) / S
    dlow, = torch.autograd.grad(z, x, dz)
    return WceRef(loss, S, bad, dlow.permute(0, 2, 3, 1).contiguous())


def wce_autograd(low, labels, weights=None, smoothing=0.0, align_corners=True, ignore_index=255):
    """(loss, dlow [B,h,w,K]) in float64 from F.cross_entropy(weight=, ignore_index=, label_smoothing=) by autograd: torch itself, which checks the
    restatement above.  (torch raises for out-of-range labels: none here.)"""
    x = _low64(low)
    lab = torch.as_tensor(np.asarray(labels)).long()
    w = None if weights is None else torch.as_tensor(np.asarray(weights)).double()
    z = F.interpolate(x, size=tuple(lab.shape[-2:]), mode="bilinear", align_corners=align_corners)
    loss = F.cross_entropy(z, lab, weight=w, ignore_index=ignore_index, label_smoothing=float(smoothing))
    loss.backward()
    return loss.detach(), x.grad.permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------------ the cases
# (B, K, (h, w), (H, W), align_corners): the smallest shapes at which the kernel can go wrong
Shape = collections.namedtuple("Shape", "name B K hw HW align_corners")
SHAPES = [
    Shape("one", 1, 3, (1, 1), (1, 1), True),
    Shape("1x1_5x3", 2, 3, (1, 1), (5, 3), True),
    Shape("k1", 1, 1, (2, 3), (4, 6), True),                        # K = 1: the loss is 0 and S the count
    Shape("ident_ac", 1, 4, (2, 2), (2, 2), True),
    Shape("ident", 1, 4, (2, 2), (2, 2), False),
    Shape("k19_ac", 2, 19, (5, 7), (33, 45), True),                 # the KT = 19 instantiation
    Shape("k19", 2, 19, (5, 7), (33, 45), False),
    Shape("k32", 1, 32, (3, 2), (7, 5), True),                      # the register-array maximum on the generic instantiation
    Shape("tiles_ac", 1, 19, (4, 40), (25, 300), True),             # several x-tiles, the last one partial, factor about 8 (97 -> 769)
    Shape("tiles", 1, 19, (4, 40), (25, 300), False),
    Shape("f32", 2, 5, (3, 3), (96, 96), True),                     # factor 32: pick_jt narrows the tile
]
SHAPE_BY_NAME = {s.name: s for s in SHAPES}
# what is switched on: class weights (one of them 0 where K > 1), label smoothing 0.1, both
VARIANTS = [("w", True, 0.0), ("s", False, 0.1), ("ws", True, 0.1)]
IGNORED_PERCENT = 20


def make_weights(key, K):
    """[K] float32 in [0.25, 2.25), one of them exactly 0 when there are at least two classes."""
    w = (synth.uniform(key + ".cw", (K,)) + 0.5) * 2.0 + 0.25
    if K > 1:
        w[int(synth.hash_u32(key + ".zero", 1)[0] % np.uint64(K))] = 0.0
    return w.astype(np.float32)


def make_inputs(key, B, K, hw, HW, ignored_percent=IGNORED_PERCENT, magnitude=None):
    """(low [B,h,w,K] float32 ~ N(0, 2), labels [B,H,W] int64 with about ignored_percent % at 255) - pure functions of `key` and the shapes.
    magnitude: the logits are scaled so that their largest magnitude is this."""
    (h, w), (H, W) = hw, HW
    low = sum(synth.uniform(key + ".low", (B, h, w, K), salt=s) for s in range(4)) * np.sqrt(6.0)
    if magnitude is not None:
        low = low * (magnitude / np.abs(low).max())
    n = B * H * W
    lab = (synth.hash_u32(key + ".lab", n) % np.uint64(K)).astype(np.int64)
    if n > 2:
        lab[(synth.hash_u32(key + ".ign", n) % np.uint64(100)) < np.uint64(ignored_percent)] = 255
        if (lab == 255).all():
            lab[0] = 0
    return low.astype(np.float32), lab.reshape(B, H, W)


def shape_inputs(shape):
    """(low, labels, weights) of one SHAPES row"""
    low, lab = make_inputs("wce." + shape.name, shape.B, shape.K, shape.hw, shape.HW)
    return low, lab, make_weights("wce." + shape.name, shape.K)
