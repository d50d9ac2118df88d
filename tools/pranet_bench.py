"""PraNet (BASELINE config[3]: configs/pranet_src_polyp.yaml, 352 x 352, batch 16) training-step throughput on one MI355X:
forward, four losses, backward, clamped Adam.

    python tools/pranet_bench.py [--batch 16] [--size 352] [--steps 20] [--graph] [--loss structure|tversky] [--boundary-weight W] [--literal] [--alternate ROUNDS]

--loss structure: the trainer's own structure loss on the four full-resolution maps (the default); --loss tversky: the Tversky + BCE compound fused
with the four heads' upsamples (configs/pranet_src_polyp_tversky.yaml, PraNet.losses).  --literal (with tversky): the composition without the fusion -
net(x) materialises the four [B,1,H,W] maps, each goes through the host/losses.py modules.
--alternate N: structure, tversky and tversky --literal one after the other, N times over, in this one process (one JSON line per variant and
round), so that the three are compared on one box under the same conditions; the peak of allocated memory is reset before every variant.
--boundary-weight W (with tversky): W times the boundary loss on the mask's signed distance map in every head (SOLVER.BOUNDARY_WEIGHT); with
--alternate the three variants become tversky without the term, with it, and with it --literal."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rnd_semantic_segmentation_amd.host import pranet, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=352)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--loss", choices=("structure", "tversky"), default="structure")
    ap.add_argument("--literal", action="store_true", help="with --loss tversky: materialised maps through the loss modules")
    ap.add_argument("--boundary-weight", type=float, default=0.0, metavar="W", help="with --loss tversky: W x the boundary loss in every head")
    ap.add_argument("--alternate", type=int, default=0, metavar="ROUNDS", help="run structure, tversky and tversky --literal in turn, ROUNDS times, in this process")
    a = ap.parse_args()
    if a.literal and a.loss != "tversky":
        ap.error("--literal goes with --loss tversky")
    if a.boundary_weight and a.loss != "tversky":
        ap.error("--boundary-weight goes with --loss tversky")
    torch.manual_seed(0)
    net = pranet.PraNet().cuda().train()
    net.ensure_flat()
    opt = pranet.FlatAdam(net, 1e-4 / 8, grad_clamp=0.5)
    img, mask = synth.synth_polyp(a.batch, a.size, a.size, seed=3)
    x, gt = torch.from_numpy(img).cuda(), torch.from_numpy(mask).cuda()

    def measure(loss_name, literal, warmup, boundary_weight=0.0):
        criterion = "ce" if loss_name == "structure" else "tversky"

        def step():
            opt.zero_grad()
            ls = pranet.step_losses(net, x, gt, criterion, literal=literal, boundary_weight=boundary_weight)
            (ls[3] + ls[2] + ls[1] + ls[0]).backward()
            opt.step()
            return ls[3]

        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        runner = step
        if a.graph:
            gs = pranet.GraphedStep(net, opt, x, gt, criterion=criterion, literal=literal, boundary_weight=boundary_weight)
            runner = lambda: gs()[3]
        for _ in range(warmup):
            loss = runner()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            loss = runner()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / a.steps
        row = {"metric": "PraNet train images/s", "value": round(a.batch / dt, 1), "ms_per_step": round(dt * 1e3, 2), "batch": a.batch, "size": a.size,
               "hip_graph": bool(a.graph), "loss_lateral2": round(float(loss.detach()), 4), "max_mem_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}
        if a.alternate or loss_name != "structure":
            row["loss_name"] = loss_name + ("-literal" if literal else "")
        if boundary_weight or a.boundary_weight:
            row["boundary_weight"] = boundary_weight
        print(json.dumps(row), flush=True)

    if a.alternate and a.boundary_weight:
        for r in range(a.alternate):
            for literal, weight in ((False, 0.0), (False, a.boundary_weight), (True, a.boundary_weight)):
                measure("tversky", literal, a.warmup if r == 0 else 1, weight)
    elif a.alternate:
        for r in range(a.alternate):
            for loss_name, literal in (("structure", False), ("tversky", False), ("tversky", True)):
                measure(loss_name, literal, a.warmup if r == 0 else 1)
    else:
        measure(a.loss, a.literal, a.warmup, a.boundary_weight)


if __name__ == "__main__":
    main()
