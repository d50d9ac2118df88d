"""What feeding real pictures costs (results: profiles/augment_bench.txt, README).

    python tools/augment_bench.py pil      # the reference's CPU transform through PIL: per image on one core, 16 processes, PNG decode apart
    python tools/augment_bench.py kernels  # mi_augment_batch on batches of 8 (run it under `rocprofv3 --kernel-trace --stats -- python ...` for per-kernel times)
    python tools/augment_bench.py loader   # DeviceAugmentLoader with 16 decode workers on a tree of PNGs written to a temporary directory
    python tools/augment_bench.py step     # the DeepLab training step on bench.py's synthetic batch against the same step fed by the loader, alternating

Plans: source 1914x1052 -> 1280x720 with all four ColorJitter ops (the reference's FADA configuration), target 2048x1024 -> 1024x512.
"""
import argparse
import io
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

SOURCE, TARGET = ((1052, 1914), (720, 1280)), ((1024, 2048), (512, 1024))
HBM_PEAK = 8.0e12          # bytes/s, MI355X


def plans(which, n, seed=0):
    from rnd_semantic_segmentation_amd.host import augment
    (H, W), (h, w) = SOURCE if which == "source" else TARGET
    spec = augment.AugmentSpec((h, w), True, jitter=(0.5, 0.5, 0.5, 0.2) if which == "source" else (0, 0, 0, 0))
    return [augment.sample_plan(spec, H, W, seed=seed, index=i) for i in range(n)]


def picture(hw, seed):
    import _augment_ref as ref
    return ref.synth_picture(hw[0], hw[1], seed, block=1), ref.synth_ids(hw[0], hw[1], seed)


def _pil_one(args):
    import _augment_ref as ref
    which, seed, reps = args
    img, lab = picture((SOURCE if which == "source" else TARGET)[0], seed)
    plan = plans(which, 1, seed)[0]
    t0 = time.perf_counter()
    for _ in range(reps):
        u8, lb = ref.run_plan_pil(img, lab, plan)
        ref.to_tensor_normalize(u8, plan)
    return (time.perf_counter() - t0) / reps


def cmd_pil(args):
    import multiprocessing as mp

    import torch
    from PIL import Image
    torch.set_num_threads(1)
    for which in ("source", "target"):
        t = min(_pil_one((which, s, 2)) for s in range(3))
        print("pil %s transform, one core: %.1f ms/image" % (which, 1000 * t))
        with mp.get_context("spawn").Pool(16) as pool:
            pool.map(_pil_one, [(which, s, 1) for s in range(16)])                      # start-up, imports
            t0 = time.perf_counter()
            pool.map(_pil_one, [(which, s, 4) for s in range(16)])
            dt = time.perf_counter() - t0
        print("pil %s transform, 16 processes: %.1f images/s" % (which, 64 / dt))
        img, _ = picture((SOURCE if which == "source" else TARGET)[0], 0)
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, "PNG")
        t0 = time.perf_counter()
        for _ in range(5):
            np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))
        print("png decode %s (%.1f MB file), one core: %.1f ms/image" % (which, len(buf.getvalue()) / 1e6, 200 * (time.perf_counter() - t0)))


def cmd_kernels(args):
    import torch
    from rnd_semantic_segmentation_amd.host import augment
    aug = augment.DeviceAugmenter("cuda", slots=1)
    for which in ("source", "target"):
        hw, out = SOURCE if which == "source" else TARGET
        pics = [picture(hw, s) for s in range(2)]
        imgs, labs, pl = [pics[i % 2][0] for i in range(8)], [pics[i % 2][1] for i in range(8)], plans(which, 8)
        for _ in range(3):
            aug(imgs, labs, pl)
        torch.cuda.synchronize()
        # the launches alone: the staged bytes are on the device already, so re-issue the kernels on the same records (grey_sum zeroed by the copy each time)
        times = []
        for _ in range(args.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            slot = aug.slots[0]
            n = 8 * 480
            slot["dev"][:n].copy_(slot["pinned"][:n], non_blocking=True)
            out_img = torch.empty((8, 3) + out, dtype=torch.float32, device="cuda")
            out_lab = torch.empty((8,) + out, dtype=torch.float32, device="cuda")
            e0.record()
            from rnd_semantic_segmentation_amd import kernels
            kernels.augment_batch(slot["dev"], slot["pinned"], 8, out_img, out_lab)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        t0 = time.perf_counter()
        for _ in range(args.iters):
            aug(imgs, labs, pl)
        torch.cuda.synchronize()
        whole = (time.perf_counter() - t0) / args.iters
        must = 8 * (hw[0] * hw[1] * 3 + out[0] * out[1] * 3 * 4)                       # raw image read once, output written once
        med = float(np.median(times))
        print("kernels %s, batch 8: median %.3f ms (min %.3f) by events; %.1f MB that must move = %.1f %% of the %.1f TB/s HBM peak; "
              "stage + copy + kernels from the host: %.1f ms/batch" % (which, med, min(times), must / 1e6, 100 * must / (med * 1e-3) / HBM_PEAK, HBM_PEAK / 1e12, 1000 * whole))


def write_tree(root, n):
    from PIL import Image
    hw = SOURCE[0]
    for sub in ("images", "labels"):
        os.makedirs(os.path.join(root, "gta5", "fold_1", sub))
    import shutil
    for i in range(n):
        paths = [os.path.join(root, "gta5", "fold_1", sub, "%05d.png" % i) for sub in ("images", "labels")]
        if i < 8:                                               # eight different pictures, repeated: encoding is not what is measured
            img, lab = picture(hw, i)
            Image.fromarray(img).save(paths[0], compress_level=3)
            Image.fromarray(lab).save(paths[1])
        else:
            for p in paths:
                shutil.copy(p.replace("%05d.png" % i, "%05d.png" % (i % 8)), p)


def gta5_cfg(root, out_wh, batch=8):
    from rnd_semantic_segmentation_amd.host import config as hc
    cfg = hc.CfgNode(hc.default_tree())
    cfg.merge_from_file(os.path.join(ROOT, "configs", "deeplabv2_r101_adv_gta5.yaml"))
    cfg.merge_from_list(["DATASETS.DATASET_DIR", root, "DATASETS.CROSS_VAL", 0, "INPUT.SOURCE_INPUT_SIZE_TRAIN", out_wh, "SOLVER.BATCH_SIZE", batch,
                         "OUTPUT_DIR", os.path.join(root, "out")])
    return cfg


def make_loader(cfg):
    from rnd_semantic_segmentation_amd.host import data, datasets
    ds = data.build_dataset(cfg, "train", True)
    return datasets.wrap_loader(ds, batch_size=cfg.SOLVER.BATCH_SIZE, shuffle=True, num_workers=16, drop_last=True)


def cmd_loader(args):
    import torch
    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        write_tree(root, args.images)
        print("wrote %d PNGs of 1914x1052 in %.1f s" % (args.images, time.perf_counter() - t0))
        loader = make_loader(gta5_cfg(root, (1280, 720)))
        for epoch in range(args.epochs):
            t0 = time.perf_counter()
            n = 0
            for img, lab, names in loader:
                n += img.shape[0]
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print("loader epoch %d: %d images in %.2f s = %.1f images/s (16 decode workers; epoch 0 includes their start-up)" % (epoch, n, dt, n / dt))


def cmd_step(args):
    import logging

    import torch
    import bench
    from rnd_semantic_segmentation_amd.host import synth
    from rnd_semantic_segmentation_amd.host.trainer import ASPPTrainer
    with tempfile.TemporaryDirectory() as root:
        write_tree(root, args.images)
        cfg = gta5_cfg(root, (769, 769))
        cfg.freeze()
        log = logging.getLogger("augment_bench")
        log.addHandler(logging.NullHandler())
        trainer = ASPPTrainer("aspp", cfg, [None] * 1000, 0, logger=log)
        with torch.no_grad():
            for m in (trainer.feature_extractor, trainer.classifier):
                synth.load_formula_weights(m)
                st = getattr(m, "_store", None)
                if st is not None:
                    st.generation += 1
        x, lab = bench.synthetic_batch(8, 769, 0, torch.device("cuda", 0))
        loader = make_loader(cfg)

        def run_synthetic(k):
            for _ in range(k):
                trainer.train_step(x, lab, 100000)
                trainer.iteration += 1

        def run_loader(k):
            done = 0
            while done < k:
                for img, lb, _ in loader:
                    trainer.train_step(img, lb, 100000)
                    trainer.iteration += 1
                    done += 1
                    if done == k:
                        break

        run_synthetic(5)
        run_loader(len(loader))
        torch.cuda.synchronize()
        for rnd in range(args.rounds):
            for name, fn, k in (("synthetic batch", run_synthetic, args.steps), ("loader attached", run_loader, len(loader) * max(1, args.steps // len(loader)))):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(k)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                print("step round %d, %s: %.2f ms/step, %.1f images/s (%d steps of 8 x 769 x 769)" % (rnd, name, 1000 * dt / k, 8 * k / dt, k))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("pil", "kernels", "loader", "step"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    {"pil": cmd_pil, "kernels": cmd_kernels, "loader": cmd_loader, "step": cmd_step}[args.what](args)


if __name__ == "__main__":
    main()
