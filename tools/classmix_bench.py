"""AsppClassMix (mean teacher + ClassMix, host/self_train.py) on one MI355X, synthetic data, R101 + ASPP with formula weights.  Not the headline
metric (bench.py is).

  (default)         one iteration at 4 + 4 crops of 512 x 1024: the fused path (mi_label_classes, mi_classmix, mi_ema_update) against
                    AsppClassMix.FUSED = False (the composition from torch ops on a materialised [B,19,H,W] probability map) and against a plain
                    ASPPTrainer step on 8 images - what the teacher pass, the mixing and the EMA cost on top.  The three ALTERNATE in one process
                    after a warm-up; the clock is read after a device synchronise; peak memory is reset before every timed call.
  --kernels N       the three kernels alone, N times at that geometry (the EMA over an R101 + head sized store), for a separate
                    `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/classmix_bench.py --kernels N` run
  --floors CSV      that run's *_kernel_stats.csv -> the three kernels' average times against their byte floors (bytes moved / HBM peak)
  --parent DIR      bench.py --gpus 1 of this tree against the tree in DIR (the parent commit, built), two alternating pairs of fresh processes

    python tools/classmix_bench.py [--iters 10] [--warmup 3]
"""
import argparse
import csv
import json
import logging
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, H, W, NC = 4, 512, 1024, 19
LOW = (65, 129)                       # the head's 1/8-resolution grid of a 512 x 1024 crop
HBM_PEAK = 8.0e12                     # bytes / s (spec); a float4 copy reaches about 6.3e12
R101_STORE = 42_500_000 + 1_400_000   # floats: the backbone's flat store + the head's, roughly (the real stores are used when models are built)


def byte_floors(n_ema):
    px = B * H * W
    low = B * LOW[0] * LOW[1] * NC * 4
    return {
        "label_classes_kernel": ("labels read once", px * 8),
        "classmix_kernel": ("label 8 + one image 12 read, image 12 + label 8 written per pixel, + the low-resolution logits", px * 40 + low),
        "ema_kernel": ("teacher read + written, student read", n_ema * 12),
    }


def timed(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, torch.cuda.max_memory_allocated() / 2 ** 30, out


def report(name, ms, mem):
    return "%-34s median %8.3f ms (min %.3f, max %.3f)   peak memory %.2f GiB" % (name, statistics.median(ms), min(ms), max(ms), max(mem))


def build_combo():
    from rnd_semantic_segmentation_amd.host import config as hc, self_train, synth, trainer
    cfg = hc.CfgNode(hc.default_tree())
    cfg.merge_from_file(os.path.join(ROOT, "configs", "deeplabv2_r101_classmix.yaml"))
    cfg.merge_from_list(["OUTPUT_DIR", os.path.join(ROOT, "build", "classmix_bench"), "SOLVER.MIX_THRESHOLD", 0.0625])
    cfg.freeze()
    self_train.setup_logger = lambda *a, **k: logging.getLogger("classmix_bench")
    combo = self_train.AsppClassMix("aspp_classmix", cfg, [], [], 0)
    for m in (combo.aspp.feature_extractor, combo.aspp.classifier):
        synth.load_formula_weights(m)
    for t, s in ((combo.teacher_feature_extractor, combo.aspp.feature_extractor), (combo.teacher_classifier, combo.aspp.classifier)):
        t.load_state_dict(s.state_dict())
    combo._teacher_changed()
    plain_cfg = hc.CfgNode(hc.default_tree())          # (the self-training keys stay at their defaults: any other trainer refuses them)
    plain_cfg.merge_from_file(os.path.join(ROOT, "configs", "deeplabv2_r101_classmix.yaml"))
    plain_cfg.merge_from_list(["OUTPUT_DIR", cfg.OUTPUT_DIR])
    plain_cfg.freeze()
    plain = trainer.ASPPTrainer("aspp", plain_cfg, [], 0, logging.getLogger("classmix_bench"))
    for m in (plain.feature_extractor, plain.classifier):
        synth.load_formula_weights(m)
    return combo, plain


def run_iterations(args):
    import torch
    from rnd_semantic_segmentation_amd.host import synth
    combo, plain = build_combo()
    xs = torch.from_numpy(synth.synth_image(B, H, W, seed=1)).cuda()
    ys = torch.from_numpy(synth.synth_label(B, H, W, NC, seed=1)).cuda()
    xt = torch.from_numpy(synth.synth_image(B, H, W, seed=2)).cuda()
    x8, y8 = torch.cat((xs, xt), 0), torch.cat((ys, ys), 0)
    max_iter = 100 * (args.warmup + args.iters)
    last = {}

    def mix(fused):
        combo.FUSED = fused
        r = combo.train_step(xs, ys, xt, max_iter)
        last[fused] = r
        return r["loss"]

    def source_only():
        loss, _ = plain.train_step(x8, y8, max_iter)
        plain.iteration += 1
        return loss

    sides = {"AsppClassMix fused": lambda: mix(True), "AsppClassMix FUSED = False": lambda: mix(False), "ASPPTrainer, 8 images": source_only}
    for _ in range(args.warmup):
        for f in sides.values():
            f()
    ms, mem = {k: [] for k in sides}, {k: [] for k in sides}
    for _ in range(args.iters):                              # alternating: drift of the clocks hits all alike
        for k, f in sides.items():
            t, m, _ = timed(f)
            ms[k].append(t)
            mem[k].append(m)
    px = B * H * W
    print("%d + %d crops of %d x %d, R101 + ASPP, formula weights, %d alternating iterations after %d warm-up:" % (B, B, H, W, args.iters, args.warmup))
    for k in sides:
        print("  " + report(k, ms[k], mem[k]))
    med = {k: statistics.median(v) for k, v in ms.items()}
    print("  FUSED = False / fused: %.3f    fused - plain step: %.3f ms (teacher forward, mixing, EMA, re-pack)" % (
        med["AsppClassMix FUSED = False"] / med["AsppClassMix fused"], med["AsppClassMix fused"] - med["ASPPTrainer, 8 images"]))
    for fused, r in sorted(last.items(), reverse=True):
        pasted, kept = (int(v) for v in r["counts"].sum(0))
        print("  last iteration, fused %-5s loss %.5f   pasted %.3f of the pixels   pseudo-labels kept on %.3f of the unpasted ones" % (
            fused, float(r["loss"]), pasted / px, kept / max(px - pasted, 1)))


def run_kernels(n):
    import torch
    from rnd_semantic_segmentation_amd import kernels
    from rnd_semantic_segmentation_amd.host import self_train, synth
    xs = torch.from_numpy(synth.synth_image(B, H, W, seed=1)).cuda()
    ys = torch.from_numpy(synth.synth_label(B, H, W, NC, seed=1)).cuda().long()
    xt = torch.from_numpy(synth.synth_image(B, H, W, seed=2)).cuda()
    g = torch.Generator().manual_seed(3)
    low = (torch.randn((B,) + LOW + (NC,), generator=g) * 3.0).cuda()
    prio = self_train.draw_priorities(0, 0, B, NC).cuda()
    teacher, student = torch.randn(R101_STORE, generator=g).cuda(), torch.randn(R101_STORE, generator=g).cuda()
    hyper = torch.tensor([0.99], device="cuda")
    out_img = torch.empty_like(xs)
    for _ in range(n + 2):
        present = kernels.label_classes(ys, NC)
        r = kernels.classmix(xs, xt, ys, low, present, prio, 0.5, 255, out_img=out_img)
        kernels.ema_update(teacher, student, hyper)
    torch.cuda.synchronize()
    pasted, kept = (int(v) for v in r.counts.sum(0))
    print(json.dumps({"kernels": n, "geometry": [B, H, W, NC], "ema_floats": R101_STORE, "pasted": pasted / (B * H * W), "kept_of_unpasted": kept / max(B * H * W - pasted, 1)}))


def run_floors(path):
    floors = byte_floors(R101_STORE)
    print("kernel times (rocprofv3 --kernel-trace --stats) against byte floors at %.1f TB/s:" % (HBM_PEAK / 1e12))
    for row in csv.DictReader(open(path)):
        for key, (what, nbytes) in floors.items():
            if key in row["Name"]:
                avg = float(row["AverageNs"]) / 1e3
                floor = nbytes / HBM_PEAK * 1e6
                print("  %-22s %4s calls   avg %8.2f us (min %.2f)   %7.1f MB (%s)   floor %7.2f us   floor / avg %.2f   %.2f TB/s" % (
                    key, row["Calls"], avg, float(row["MinNs"]) / 1e3, nbytes / 1e6, what, floor, floor / avg, nbytes / avg / 1e6))


def run_parent(args):
    trees = [("this tree", ROOT), ("parent", os.path.abspath(args.parent))]
    vals = {k: [] for k, _ in trees}
    for pair in range(2):
        for name, root in trees:                              # alternating pairs, a fresh process each
            p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(args.steps), "--warmup", str(args.bench_warmup)],
                               cwd=root, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                print("bench.py of %s failed (%d): %s" % (name, p.returncode, p.stderr[-2000:]))
                sys.exit(1)          # nothing more is started on the GPU after a failure
            out = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            vals[name].append(out["value"])
            print("  pair %d  %-9s %s %.2f %s" % (pair + 1, name, out["metric"], out["value"], out["unit"]))
    a, b = statistics.mean(vals["this tree"]), statistics.mean(vals["parent"])
    print("  bench.py --gpus 1 --steps %d --warmup %d: this tree %.2f, parent %.2f images/s (this / parent %.4f)" % (args.steps, args.bench_warmup, a, b, a / b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernels", type=int, default=0)
    ap.add_argument("--floors", default="")
    ap.add_argument("--parent", default="")
    ap.add_argument("--steps", type=int, default=20, help="with --parent: bench.py --steps")
    ap.add_argument("--bench-warmup", type=int, default=5, help="with --parent: bench.py --warmup")
    args = ap.parse_args()
    if args.floors:
        run_floors(args.floors)
    elif args.kernels:
        run_kernels(args.kernels)
    elif args.parent:
        run_parent(args)
    else:
        run_iterations(args)


if __name__ == "__main__":
    main()
