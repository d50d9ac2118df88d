"""A plain torch restatement of the locally connected CRF refinement (TEST.CRF; the definition: include/mi355seg.h, mi_crf_refine), built from
shifted slices.  float64 is the oracle of tests/test_gpu_crf.py, float32 the yardstick for rounding: the kernel may deviate from the oracle by
CRF_FACTOR times what this restatement itself deviates when it runs in float32.  crf_brute is the same formula as a per-pixel double loop in
Python floats (tests/test_host_crf.py checks the restatement against it)."""
import math

import numpy as np
import torch

EPS = 1e-5
CRF_FACTOR = 16.0          # kernel bound = CRF_FACTOR * max|float32 restatement - float64 oracle| on the same case
DEFAULTS = dict(iters=5, window=7, dilation=4, pos_w=3.0, pos_xy=3.0, bi_w=10.0, bi_xy=80.0, bi_rgb=13.0)


def _offsets(window, dilation):
    r = window // 2
    return [(dy * dilation, dx * dilation) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if (dy, dx) != (0, 0)]      # row-major


def _shift(t, oy, ox):
    """out[..., y, x] = t[..., y + oy, x + ox] where that pixel lies inside the image, else 0; None when no pixel has such a neighbour."""
    H, W = t.shape[-2:]
    y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
    if y0 >= y1 or x0 >= x1:
        return None
    out = torch.zeros_like(t)
    out[..., y0:y1, x0:x1] = t[..., y0 + oy:y1 + oy, x0 + ox:x1 + ox]
    return out


def crf_weights(image, cs, window, dilation, pos_w, pos_xy, bi_w, bi_xy, bi_rgb, dtype):
    """[(oy, ox, k)] with k [B,1,H,W] = k(i, o) of the definition, for the offsets that have any pixel inside."""
    I = image.to(dtype)
    B, _, H, W = I.shape
    scale = torch.tensor([float(v) for v in cs], dtype=dtype).reshape(1, 3, 1, 1)
    ones = torch.ones((B, 1, H, W), dtype=dtype)
    taps = []
    Np = torch.zeros((B, 1, H, W), dtype=dtype)
    Nb = torch.zeros((B, 1, H, W), dtype=dtype)
    for oy, ox in _offsets(window, dilation):
        inside = _shift(ones, oy, ox)
        if inside is None:
            continue
        o2 = torch.tensor(float(oy * oy + ox * ox), dtype=dtype)
        gp = torch.exp(-o2 / (2 * pos_xy ** 2))
        gb = torch.exp(-o2 / (2 * bi_xy ** 2))
        diff = (scale * (_shift(I, oy, ox) - I)) ** 2
        gc = torch.exp(-(diff[:, 0:1] + diff[:, 1:2] + diff[:, 2:3]) / (2 * bi_rgb ** 2))
        Np = Np + inside * gp
        Nb = Nb + inside * gb
        taps.append((oy, ox, inside, gp, gb, gc))
    zero = torch.zeros((), dtype=dtype)
    out = []
    for oy, ox, inside, gp, gb, gc in taps:
        kp = torch.where(Np > 0, pos_w * gp / torch.where(Np > 0, Np, ones), zero)
        kb = torch.where(Nb > 0, bi_w * gb * gc / torch.where(Nb > 0, Nb, ones), zero)
        out.append((oy, ox, inside * (kp + kb)))
    return out


def crf_ref(probs, image, cs, iters, window, dilation, pos_w, pos_xy, bi_w, bi_xy, bi_rgb, dtype=torch.float64):
    """Q^{iters} [B,K,H,W] in `dtype` on the CPU from probs [B,K,H,W] and image [B,3,H,W]."""
    p = probs.detach().cpu().to(dtype)
    U = torch.log(torch.clamp(p, min=EPS))
    Q = torch.softmax(U, dim=1)
    if iters == 0:
        return Q
    taps = crf_weights(image.detach().cpu(), cs, window, dilation, pos_w, pos_xy, bi_w, bi_xy, bi_rgb, dtype)
    for _ in range(iters):
        msg = torch.zeros_like(Q)
        for oy, ox, k in taps:
            msg = msg + k * _shift(Q, oy, ox)
        Q = torch.softmax(U + msg, dim=1)
    return Q


def crf_brute(probs, image, cs, iters, window, dilation, pos_w, pos_xy, bi_w, bi_xy, bi_rgb):
    """The definition as written, one pixel and one neighbour at a time, in Python floats: numpy float64 [K,H,W] from [K,H,W] and [3,H,W]."""
    p, I = np.asarray(probs, dtype=np.float64), np.asarray(image, dtype=np.float64)
    K, H, W = p.shape
    offsets = _offsets(window, dilation)

    def softmax(v):
        m = max(v)
        e = [math.exp(x - m) for x in v]
        s = sum(e)
        return [x / s for x in e]

    U = [[[math.log(max(float(p[c, y, x]), EPS)) for c in range(K)] for x in range(W)] for y in range(H)]
    Q = [[softmax(U[y][x]) for x in range(W)] for y in range(H)]
    for _ in range(iters):
        new = [[None] * W for _ in range(H)]
        for y in range(H):
            for x in range(W):
                inside = [(oy, ox) for oy, ox in offsets if 0 <= y + oy < H and 0 <= x + ox < W]
                Np = sum(math.exp(-(oy * oy + ox * ox) / (2 * pos_xy ** 2)) for oy, ox in inside)
                Nb = sum(math.exp(-(oy * oy + ox * ox) / (2 * bi_xy ** 2)) for oy, ox in inside)
                msg = [0.0] * K
                for oy, ox in inside:
                    o2 = oy * oy + ox * ox
                    d2 = sum((cs[ch] * (float(I[ch, y + oy, x + ox]) - float(I[ch, y, x]))) ** 2 for ch in range(3))
                    k = 0.0
                    if Np > 0:
                        k += pos_w * math.exp(-o2 / (2 * pos_xy ** 2)) / Np
                    if Nb > 0:
                        k += bi_w * math.exp(-o2 / (2 * bi_xy ** 2)) * math.exp(-d2 / (2 * bi_rgb ** 2)) / Nb
                    for c in range(K):
                        msg[c] += k * Q[y + oy][x + ox][c]
                new[y][x] = softmax([U[y][x][c] + msg[c] for c in range(K)])
        Q = new
    return np.array(Q, dtype=np.float64).transpose(2, 0, 1)


def crf_inputs(K, B, H, W, seed, cs=(58.395, 57.12, 57.375), noise=8.0, bias=2.0):
    """(probs [B,K,H,W], image [B,3,H,W]) float32 on the CPU: a piecewise-constant image (blocks of about a quarter of the shorter side, one colour
    per region) with Gaussian noise of sigma `noise` in 0..255 units, divided by cs (the normalised tensor the tester holds); probabilities =
    softmax of random logits with `bias` added to the class of the pixel's region - the CRF then moves a real share of the pixels."""
    g = torch.Generator().manual_seed(seed)
    blk = max(1, min(H, W) // 4)
    ny, nx = (H + blk - 1) // blk, (W + blk - 1) // blk
    region = torch.randint(0, K, (B, ny, nx), generator=g)
    region = region.repeat_interleave(blk, 1)[:, :H].repeat_interleave(blk, 2)[:, :, :W]                    # [B,H,W]
    colours = torch.rand((K, 3), generator=g) * 255.0
    img = colours[region].permute(0, 3, 1, 2) + noise * torch.randn((B, 3, H, W), generator=g)
    img = (img / torch.tensor(cs).reshape(1, 3, 1, 1)).float().contiguous()
    logits = 1.5 * torch.randn((B, K, H, W), generator=g)
    logits = logits + bias * torch.nn.functional.one_hot(region, K).permute(0, 3, 1, 2)
    return torch.softmax(logits, 1).float().contiguous(), img
