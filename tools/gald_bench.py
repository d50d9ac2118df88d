"""GALD (HarDNet-68 + GCPA decoder; configs/gald_src.yaml: batch 6, 1280 x 720 crops) training-step throughput on one MI355X: encoder + decoder forward,
four head losses, backward, both Adam steps.

    python tools/gald_bench.py [--batch 6] [--height 720] [--width 1280] [--steps 10] [--loss ce|gdl|ohem|lovasz] [--literal] [--alternate ROUNDS]
                               [--class-weights median] [--label-smoothing S] [--ohem-thresh T] [--ohem-min-kept M] [--focal-gamma G] [--lovasz-ce W]

--loss ce: the four fused upsample + cross-entropy heads (the default); --loss gdl: the four fused upsample + generalized Dice heads
(configs/gald_src_dice.yaml).  --literal (with gdl): the composition without the fused kernel - decoder(x, feats) materialises the four [B,19,H,W]
outputs, each goes as fp32 NCHW through the reference's GeneralizedDiceLoss written with torch ops, autograd does the backward.
--class-weights median / --label-smoothing S (with ce): CrossEntropyLoss(weight=, label_smoothing=) inside the fused heads (mi_upsample_ce_w), the
weights by median-frequency balancing (tools/class_weights.py) of the bench's own labels; with --literal: the four materialised outputs through
F.cross_entropy(weight=, label_smoothing=) with autograd.
--loss ohem: the four fused upsample + cross-entropy heads with online hard example mining (mi_upsample_ce_ohem; configs/gald_src_ohem.yaml), each head
keeping the pixels whose probability of the true class is at most max(T, the M-th smallest of the head); with --literal: the four materialised outputs
through a torch-op OHEM (softmax, gather, torch.kthvalue, masked F.cross_entropy) with autograd.  With --alternate the variants are ce, ohem and
ohem --literal.
--focal-gamma G (with ce, combinable with --class-weights): the focal loss -w_y (1 - p_y)^G log p_y inside the fused heads (mi_upsample_ce_focal;
configs/gald_src_focal.yaml); with --literal: the four materialised outputs through a focal loss written with F.log_softmax / gather / pow and
autograd.  With --alternate the variants are ce, ce-focal and ce-focal --literal.
--loss lovasz: the four fused upsample + Lovasz-Softmax heads (mi_upsample_lovasz; configs/gald_src_lovasz.yaml) plus W (--lovasz-ce, default 1) times
the plain fused cross-entropy of each head; with --literal: the four materialised outputs through metrics.LovaszSoftmax (softmax and 19 torch.sort
calls per head, autograd through the gather) plus W * F.cross_entropy.  With --alternate the variants are ce, lovasz and lovasz --literal.
--alternate N: ce, gdl and gdl --literal - and, when weights or smoothing are given, ce weighted fused and ce weighted literal - one after the other, N
times over, in this one process (one JSON line per variant and round), so that they are compared on one box under the same conditions; the peak of
allocated memory is reset before every variant."""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import class_weights as cw  # noqa: E402  (tools/class_weights.py)
from rnd_semantic_segmentation_amd.host import gald, metrics, pranet, synth  # noqa: E402


def torch_gdl(output, target, eps=1e-5, weight_type="square", ignore_label=255):
    """GeneralizedDiceLoss of utility.py:399-447 (label form) with torch ops on a materialised [N,C,H,W] tensor; `target` is left as it is."""
    C = output.shape[1]
    p = torch.softmax(output, 1)
    m = target != ignore_label
    p = p * m.unsqueeze(1)
    t = F.one_hot(torch.where(m, target, torch.full_like(target, C)), C + 1)[..., :C].permute(0, 3, 1, 2)
    ts = t.sum((0, 2, 3))
    if weight_type == "square":
        w = 1. / (ts * ts + eps)
    elif weight_type == "identity":
        w = 1. / (ts + eps)
    else:
        w = 1. / (torch.sqrt(ts.float()) + eps)
    inter = ((p * t).sum((0, 2, 3)) * w).sum()
    den = ((p * p + t * t).sum((0, 2, 3)) * w).sum() + eps
    return 1 - 2. * inter / den


def torch_ohem(output, target, thresh, min_kept, ignore_label=255):
    """OhemCrossEntropy2d as GALDNet / CCNet publish it, with torch ops on a materialised [N,C,H,W] tensor: the kept set is a constant (no_grad)."""
    with torch.no_grad():
        valid = target != ignore_label
        q = torch.softmax(output, 1).gather(1, torch.where(valid, target, torch.zeros_like(target)).unsqueeze(1)).squeeze(1)[valid]
        t = torch.clamp(torch.kthvalue(q, min(min_kept, q.numel())).values, min=thresh) if q.numel() else thresh
        kept = torch.zeros_like(valid)
        kept[valid] = q <= t
    return F.cross_entropy(output, torch.where(kept, target, torch.full_like(target, ignore_label)), ignore_index=ignore_label)


def torch_focal(output, target, gamma, weight=None, ignore_label=255):
    """Focal loss -w_y (1 - p_y)^gamma log p_y over the valid pixels, divided by their weight sum, with torch ops on a materialised [N,C,H,W] tensor."""
    valid = target != ignore_label
    y = torch.where(valid, target, torch.zeros_like(target))
    logq = F.log_softmax(output, 1).gather(1, y.unsqueeze(1)).squeeze(1)
    wy = valid.to(output.dtype) if weight is None else weight[y] * valid
    u = (1.0 - logq.exp()).clamp_min(torch.finfo(output.dtype).tiny)
    return -(wy * torch.pow(u, gamma) * logq).sum() / wy.sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=6)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loss", choices=("ce", "gdl", "ohem", "lovasz"), default="ce")
    ap.add_argument("--literal", action="store_true", help="materialised outputs through a torch-op Dice loss / F.cross_entropy with autograd")
    ap.add_argument("--alternate", type=int, default=0, metavar="ROUNDS", help="run the variants in turn, ROUNDS times, in this process")
    ap.add_argument("--class-weights", choices=("median",), default=None, help="with ce: median-frequency class weights from the bench's own labels")
    ap.add_argument("--label-smoothing", type=float, default=0.0, metavar="S", help="with ce: CrossEntropyLoss's label_smoothing")
    ap.add_argument("--ohem-thresh", type=float, default=0.7, metavar="T", help="with ohem: SOLVER.OHEM_THRESH")
    ap.add_argument("--ohem-min-kept", type=int, default=100000, metavar="M", help="with ohem: SOLVER.OHEM_MIN_KEPT")
    ap.add_argument("--focal-gamma", type=float, default=0.0, metavar="G", help="with ce: SOLVER.FOCAL_GAMMA (combinable with --class-weights)")
    ap.add_argument("--lovasz-ce", type=float, default=1.0, metavar="W", help="with lovasz: SOLVER.LOVASZ_CE, the weight of the cross-entropy term")
    a = ap.parse_args()
    focal = a.focal_gamma > 0.0
    if focal and (a.loss != "ce" or a.label_smoothing != 0.0):
        ap.error("--focal-gamma goes with --loss ce and without --label-smoothing")
    weighted = (a.class_weights is not None or a.label_smoothing != 0.0) and not focal
    if weighted and a.loss != "ce" and not a.alternate:
        ap.error("--class-weights / --label-smoothing go with --loss ce")
    torch.manual_seed(0)
    enc, dec = gald.GCPAEncoder().cuda().train(), gald.GCPADecoder().cuda().train()
    enc.ensure_flat()
    dec.ensure_flat()
    oe, od = pranet.FlatAdam(enc, 1e-4), pranet.FlatAdam(dec, 1e-3)
    x = torch.from_numpy(synth.synth_image(a.batch, a.height, a.width, seed=9)).cuda()
    lab_host = synth.synth_label(a.batch, a.height, a.width, 19, seed=9)
    lab = torch.from_numpy(lab_host).cuda().long()
    weights = None
    if a.class_weights == "median":
        weights = torch.tensor(cw.class_weights(*cw.count_labels(lab_host, 19), "median"), dtype=torch.float32).cuda()

    def step(loss_name, literal):
        oe.zero_grad()
        od.zero_grad()
        extra = {"class_weights": weights, "label_smoothing": a.label_smoothing} if loss_name == "ce-weighted" else {}
        if loss_name == "ce-focal":
            extra = {"class_weights": weights, "focal_gamma": a.focal_gamma}
        if literal and loss_name == "ce-focal":
            l5, l4, l3, l2 = [torch_focal(o.float().contiguous(), lab, a.focal_gamma, weights) for o in dec(x, enc(x))]
        elif literal and loss_name == "gdl":
            l5, l4, l3, l2 = [torch_gdl(o.float().contiguous(), lab) for o in dec(x, enc(x))]
        elif literal and loss_name == "ohem":
            l5, l4, l3, l2 = [torch_ohem(o.float().contiguous(), lab, a.ohem_thresh, a.ohem_min_kept) for o in dec(x, enc(x))]
        elif loss_name == "ohem":
            l5, l4, l3, l2 = dec.losses(x, enc(x), lab, criterion="ohem", ohem=(a.ohem_thresh, a.ohem_min_kept))
        elif literal and loss_name == "lovasz":
            outs = [o.float().contiguous() for o in dec(x, enc(x))]
            l5, l4, l3, l2 = [metrics.LovaszSoftmax(o, lab) + (a.lovasz_ce * F.cross_entropy(o, lab, ignore_index=255) if a.lovasz_ce > 0 else 0.0)
                              for o in outs]
        elif loss_name == "lovasz":
            l5, l4, l3, l2 = dec.losses(x, enc(x), lab, criterion="lovasz", lovasz=a.lovasz_ce)
        elif literal:
            l5, l4, l3, l2 = [F.cross_entropy(o.float().contiguous(), lab, weight=extra.get("class_weights"), ignore_index=255,
                                              label_smoothing=extra.get("label_smoothing", 0.0)) for o in dec(x, enc(x))]
        else:
            l5, l4, l3, l2 = dec.losses(x, enc(x), lab, criterion="ce" if loss_name.startswith("ce") else loss_name, **extra)      # the trainer's path: fused
        loss = l2 * 1 + l3 * 0.8 + l4 * 0.6 + l5 * 0.4
        loss.backward()
        oe.step()
        od.step()
        return loss

    def measure(loss_name, literal, warmup):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        for _ in range(warmup):
            loss = step(loss_name, literal)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            loss = step(loss_name, literal)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / a.steps
        print(json.dumps({"metric": "GALD train images/s", "value": round(a.batch / dt, 2), "ms_per_step": round(dt * 1e3, 2), "batch": a.batch,
                          "size": [a.height, a.width], "loss_name": loss_name + ("-literal" if literal else ""), "loss": round(float(loss.detach()), 4),
                          "max_mem_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}), flush=True)

    if a.alternate:
        for r in range(a.alternate):
            variants = (("ce", False), ("gdl", False), ("gdl", True)) + ((("ce-weighted", False), ("ce-weighted", True)) if weighted else ())
            if a.loss == "ohem":
                variants = (("ce", False), ("ohem", False), ("ohem", True))
            if focal:
                variants = (("ce", False), ("ce-focal", False), ("ce-focal", True))
            if a.loss == "lovasz":
                variants = (("ce", False), ("lovasz", False), ("lovasz", True))
            for loss_name, literal in variants:
                measure(loss_name, literal, a.warmup if r == 0 else 1)
    else:
        measure("ce-focal" if focal else "ce-weighted" if weighted else a.loss, a.literal, a.warmup)


if __name__ == "__main__":
    main()
