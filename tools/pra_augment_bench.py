"""What feeding Kvasir pictures to PraNet costs (results: profiles/pra_augment_bench.txt, README); the sibling of tools/augment_bench.py for
the `pra` transform.

    python tools/pra_augment_bench.py pil      # the PIL oracle of tests/_pra_ref.py on one core, per image
    python tools/pra_augment_bench.py kernels  # mi_augment_pra_batch on a batch of 16 (under `rocprofv3 --kernel-trace --stats -- python ...` for per-kernel times)
    python tools/pra_augment_bench.py loader   # DeviceAugmentLoader with 16 decode workers on a Kvasir tree of PNGs written to a temporary directory
    python tools/pra_augment_bench.py step     # the PraNet training step on the synthetic batch against the same step fed by the loader, alternating

Pictures: 16 synthetic ones of Kvasir-SEG-like sizes, 332x487 up to 1072x1920, to 352x352.  Plans: every stage drawn (a rotation, a flip, HSV,
brightness / contrast, the transpose, a random 220 crop), and the same without the crop (the whole frame is gathered, coloured and resized:
the most work a sample can ask for).
"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

SIZES = [(332 + (1072 - 332) * i // 15, 487 + (1920 - 487) * i // 15) for i in range(16)]
OUT = 352
HBM_PEAK = 8.0e12          # bytes/s, MI355X


def plans(crop, seed=0):
    from rnd_semantic_segmentation_amd.host import pra_augment as P
    spec = P.PraSpec((OUT, OUT), True)
    out = []
    for i, (h, w) in enumerate(SIZES):
        dr = P.draw_pra(seed, 0, i)._replace(rot=True, k=1 + 2 * (i % 2), flip=True, hsv=True, bc=True, transpose=i % 4 < 2, crop=crop, center=False)
        out.append(P.plan_from_draws(spec, h, w, dr))
    return out


def pictures():
    import _pra_ref as ref
    return [(ref.synth_picture(h, w, i, block=1), ref.synth_mask(h, w, i)) for i, (h, w) in enumerate(SIZES)]


def cmd_pil(args):
    import torch
    import _pra_ref as ref
    torch.set_num_threads(1)
    pics = pictures()
    for crop in (True, False):
        times = []
        for (img, mask), plan in zip(pics, plans(crop)):
            best = 1e9
            for _ in range(2):
                t0 = time.perf_counter()
                u8, mk = ref.run_plan_pil(img, mask, plan)
                ref.to_tensor_normalize(u8, plan)
                best = min(best, time.perf_counter() - t0)
            times.append(best)
        print("pil %s, one core: mean %.1f ms/image (smallest picture %.1f, largest %.1f)" % (
            "every stage drawn" if crop else "every stage but the crop", 1000 * np.mean(times), 1000 * times[0], 1000 * times[-1]))


def cmd_kernels(args):
    import torch
    from rnd_semantic_segmentation_amd import kernels
    from rnd_semantic_segmentation_amd.host import augment
    aug = augment.DeviceAugmenter("cuda", slots=1)
    pics = pictures()
    imgs, masks = [p[0] for p in pics], [p[1] for p in pics]
    for crop in (True, False):
        pl = plans(crop)
        for _ in range(3):
            aug(imgs, masks, pl)
        torch.cuda.synchronize()
        slot = aug.slots[0]
        out_img = torch.empty((16, 3, OUT, OUT), dtype=torch.float32, device="cuda")
        out_mask = torch.empty((16, OUT, OUT), dtype=torch.float32, device="cuda")
        times = []
        for _ in range(args.iters):                                 # the launches alone, on the records already staged
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            kernels.augment_pra_batch(slot["dev"], slot["pinned"], 16, out_img, out_mask)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        t0 = time.perf_counter()
        for _ in range(args.iters):
            aug(imgs, masks, pl)
        torch.cuda.synchronize()
        whole = (time.perf_counter() - t0) / args.iters
        must = sum(p.wh * p.ww * 4 for p in pl) + 16 * OUT * OUT * 4 * 4      # window of image and mask read once, outputs written once
        med = float(np.median(times))
        print("kernels %s, batch 16: median %.3f ms (min %.3f) by events; %.1f MB that must move = %.2f %% of the %.1f TB/s HBM peak; "
              "stage + copy + kernels from the host: %.1f ms/batch" % ("every stage drawn" if crop else "every stage but the crop", med, min(times), must / 1e6,
                                                                       100 * must / (med * 1e-3) / HBM_PEAK, HBM_PEAK / 1e12, 1000 * whole))


def write_tree(root, n):
    import shutil

    from PIL import Image
    for sub in ("images", "masks"):
        os.makedirs(os.path.join(root, "kvasir", "fold_1", sub))
    pics = pictures()
    for i in range(n):
        paths = [os.path.join(root, "kvasir", "fold_1", sub, "%05d.png" % i) for sub in ("images", "masks")]
        if i < 16:                                              # sixteen different pictures, repeated: encoding is not what is measured
            Image.fromarray(pics[i][0]).save(paths[0], compress_level=3)
            Image.fromarray(pics[i][1]).save(paths[1])
        else:
            for p in paths:
                shutil.copy(p.replace("%05d.png" % i, "%05d.png" % (i % 16)), p)


def make_loader(root, batch=16):
    from rnd_semantic_segmentation_amd.host import config as hc
    from rnd_semantic_segmentation_amd.host import data, datasets
    cfg = hc.CfgNode(hc.default_tree())
    cfg.merge_from_file(os.path.join(ROOT, "configs", "pranet_src_kvasir.yaml"))
    cfg.merge_from_list(["DATASETS.DATASET_DIR", root, "DATASETS.CROSS_VAL", 0, "SOLVER.BATCH_SIZE", batch])
    ds = data.build_dataset(cfg, "train", True)
    return datasets.wrap_loader(ds, batch_size=batch, shuffle=True, num_workers=16, drop_last=True)


def cmd_loader(args):
    import torch
    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        write_tree(root, args.images)
        print("wrote %d PNG pairs of %dx%d .. %dx%d in %.1f s" % ((args.images,) + SIZES[0] + SIZES[-1] + (time.perf_counter() - t0,)))
        loader = make_loader(root)
        for epoch in range(args.epochs):
            t0 = time.perf_counter()
            n = 0
            for img, mask, names in loader:
                n += img.shape[0]
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print("loader epoch %d: %d images in %.2f s = %.1f images/s (16 decode workers; epoch 0 includes their start-up)" % (epoch, n, dt, n / dt))


def cmd_step(args):
    import torch
    from rnd_semantic_segmentation_amd.host import pranet, synth
    torch.manual_seed(0)
    net = pranet.PraNet().cuda().train()
    net.ensure_flat()
    opt = pranet.FlatAdam(net, 1e-4 / 8, grad_clamp=0.5)
    img, mask = synth.synth_polyp(16, OUT, OUT, seed=3)
    x, gt = torch.from_numpy(img).cuda(), torch.from_numpy(mask).cuda()
    step = pranet.GraphedStep(net, opt, x, gt)
    with tempfile.TemporaryDirectory() as root:
        write_tree(root, args.images)
        loader = make_loader(root)

        def run_synthetic(k):
            for _ in range(k):
                step(x, gt)

        def run_loader(k):
            done = 0
            while done < k:
                for im, mk, _ in loader:
                    step(im, mk.unsqueeze(1))
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
                print("step round %d, %s: %.2f ms/step, %.1f images/s (%d steps of 16 x %d x %d)" % (rnd, name, 1000 * dt / k, 16 * k / dt, k, OUT, OUT))


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
