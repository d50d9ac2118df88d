"""Writes tests/golden/g15_*.npz: inputs, plans and PIL results of the `aspp` input transform (tests/_augment_ref.py is the oracle:
a plan executed with PIL calls).  Needs PIL; the GPU tests read the fixtures only.

    python tools/make_augment_golden.py [--out tests/golden]

Every file is one batch (its samples agree in output size, not in source size).  A sample stores the index of its source picture, its
plan as arrays, the uint8 image as it enters ToTensor and the label; the float32 expectation is ToTensor + Normalize (torch, CPU) of
that uint8 image, recomputed by the test - three float planes per sample would make the fixtures megabytes.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import argparse  # noqa: E402
import zipfile  # noqa: E402

import numpy as np  # noqa: E402

import _augment_ref as ref  # noqa: E402
from rnd_semantic_segmentation_amd.host import augment as A  # noqa: E402
from rnd_semantic_segmentation_amd.host import datasets  # noqa: E402

B, C, S, H = A.OP_BRIGHTNESS, A.OP_CONTRAST, A.OP_SATURATION, A.OP_HUE
IMAGENET = dict(to_bgr255=False, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
CAFFE = dict(to_bgr255=True, mean=(104.00698793, 116.66876762, 122.67891434), std=(1.0, 1.0, 1.0))
T19 = datasets.id_table(datasets.TRAINID_19)
T16 = datasets.id_table(datasets.TRAINID_16)


def save(out, name, **arrays):
    """np.savez_compressed with a constant member timestamp (numpy stamps the current time: archives would differ run to run)."""
    path = os.path.join(out, name + ".npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(arrays):
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            with zf.open(info, "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(arrays[key]), allow_pickle=False)
    print("  wrote %-24s %7.1f KB" % (name + ".npz", os.path.getsize(path) / 1024))


def resize_plan(src, ops, out, flip=0, norm=IMAGENET, table=T19):
    h, w = src
    return A.Plan(h, w, ops, out[0], out[1], 0, 0, 0, 0, flip, out[0], out[1], label_table=table, **norm)


def scale_plan(src, ops, scaled, crop, out, flip=0, norm=IMAGENET, table=T19):
    """RandomScale to `scaled`, RandomCrop(out, pad_if_needed=True) at offset `crop` of the padded image."""
    h, w = src
    pad_y, pad_x = max(out[0] - scaled[0], 0), max(out[1] - scaled[1], 0)
    return A.Plan(h, w, ops, scaled[0], scaled[1], pad_y, pad_x, crop[0], crop[1], flip, out[0], out[1], label_table=table, **norm)


def test_plan(src, out, norm=IMAGENET, table=T19):
    h, w = src
    return A.Plan(h, w, [], out[0], out[1], 0, 0, 0, 0, 0, out[0], out[1], label_table=table, lab_sh=h, lab_sw=w, lab_h=h, lab_w=w, **norm)


def write(out, name, sources, samples):
    arrays = {"n": np.array(len(samples))}
    pics = {}
    for i, (hw, seed) in enumerate(sources):
        pics[i] = (ref.synth_picture(hw[0], hw[1], seed), ref.synth_ids(hw[0], hw[1], seed))
        arrays["img%d" % i], arrays["lab%d" % i] = pics[i]
    for i, (src, plan) in enumerate(samples):
        img, lab = pics[src]
        assert img.shape[:2] == (plan.H, plan.W)
        exp_img, exp_lab = ref.run_plan_pil(img, lab, plan)
        assert exp_img.shape == (plan.out_h, plan.out_w, 3) and exp_lab.shape == (plan.lab_h, plan.lab_w)
        got_img, got_lab = ref.run_plan_numpy(img, lab, plan)             # the restatement the kernels follow must agree before a fixture is written
        assert np.array_equal(got_img, exp_img) and np.array_equal(got_lab, exp_lab), (name, i)
        assert np.array_equal(exp_lab, exp_lab.astype(np.uint8))
        pre = "s%d_" % i
        arrays[pre + "src"] = np.array(src)
        arrays[pre + "exp_img"] = exp_img
        arrays[pre + "exp_lab"] = exp_lab.astype(np.uint8)
        for k, v in plan.to_arrays().items():
            arrays[pre + k] = v
    save(out, name, **arrays)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    out = ap.parse_args().out
    a, b, c, d, e = (260, 480), (200, 360), (60, 100), (100, 300), (150, 180)
    O = (100, 180)
    # colour ops: each alone below and above 1 (hue: negative and positive), all four in two orders; bicubic down to 100x180; two source sizes
    write(out, "g15_jitter", [(a, 1), (b, 2)], [
        (0, resize_plan(a, [(B, 0.6)], O)), (1, resize_plan(b, [(B, 1.4)], O, flip=1)),
        (0, resize_plan(a, [(C, 0.7)], O)), (1, resize_plan(b, [(C, 1.35)], O)),
        (0, resize_plan(a, [(S, 0.5)], O, flip=1)), (1, resize_plan(b, [(S, 1.5)], O)),
        (0, resize_plan(a, [(H, -0.07)], O)), (1, resize_plan(b, [(H, 0.05)], O)),
        (0, resize_plan(a, [(B, 0.8), (C, 0.75), (S, 0.6), (H, -0.15)], O)),
        (1, resize_plan(b, [(S, 1.3), (H, 0.2), (B, 1.2), (C, 1.45)], O, flip=1)),
    ])
    # geometry: down, up, one axis unchanged (each way), RandomScale 0.3 padded on both axes, RandomScale 1.5 cropped off-origin and mirrored,
    # both passes skipped (a plain crop of the jittered source)
    write(out, "g15_geometry", [(a, 3), (b, 4), (c, 5), (d, 6), (e, 7)], [
        (0, resize_plan(a, [], O)), (2, resize_plan(c, [], O, flip=1)), (3, resize_plan(d, [], O)), (4, resize_plan(e, [(C, 1.2)], O)),
        (0, scale_plan(a, [], (78, 144), (7, 19), O)), (0, scale_plan(a, [(S, 0.7)], (78, 144), (20, 5), O, flip=1)),
        (1, scale_plan(b, [], (300, 540), (83, 211), O, flip=1)), (1, scale_plan(b, [(H, 0.1), (C, 0.8)], (300, 540), (200, 360), O)),
        (0, scale_plan(a, [(B, 1.1)], a, (50, 121), O)),
        (4, scale_plan(e, [], (90, 108), (3, 33), O, table=T16)),
    ])
    # TO_BGR255 with the Caffe mean (the reference's commented alternative), 19- and 16-class tables
    write(out, "g15_bgr255", [(b, 8), (c, 9)], [
        (0, resize_plan(b, [], O, norm=CAFFE)), (1, resize_plan(c, [(S, 1.2), (B, 0.9)], O, flip=1, norm=CAFFE, table=T16)),
        (0, scale_plan(b, [], (300, 540), (10, 300), O, norm=CAFFE)),
    ])
    # test mode: the image resized, the label left at its own size
    write(out, "g15_test", [((120, 200), 10), ((120, 200), 11)], [
        (0, test_plan((120, 200), (64, 112))), (1, test_plan((120, 200), (64, 112), norm=CAFFE, table=T16)),
    ])


if __name__ == "__main__":
    main()
