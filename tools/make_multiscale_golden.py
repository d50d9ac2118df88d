"""Writes tests/golden/g14_*.npz: the REFERENCE's multi_scale_inference (core/utils/utility.py:193-209) on the CPU, on formula
weights and synth inputs, for the cases tests/test_multiscale_host.py and tests/test_gpu_multiscale.py compare against.

    python tools/make_multiscale_golden.py [--out tests/golden] [--only tiny|r101]

Uses oracle/make_golden.py for the import stubs, the reference nets and the per-image evaluation record; reads the reference
tree only (no bytecode is written into it) and copies none of its text.  The archives carry a fixed timestamp, so a second run
reproduces them byte for byte.

Per case: `probs` (the tiny net: the full [1,19,65,97] tensor) or `probs_crop` + `crop` (y0, y1, x0, x1), `pred` (uint8 argmax
mask), and oracle.make_golden.eval_record's iu / cmt / summary / margin_idx / margin_val (the 4096 smallest top-2 margins).
"""
import sys

sys.dont_write_bytecode = True

import argparse  # noqa: E402
import os  # noqa: E402
import zipfile  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import make_golden as mg  # noqa: E402
from rnd_semantic_segmentation_amd.host import synth  # noqa: E402

SCALE_SETS = {"s07_10_13": [0.7, 1.0, 1.3], "s05_10_175": [0.5, 1.0, 1.75]}
# (name, (H, W), seed, crop y0 y1 x0 x1): input size = label size
R101_CASES = [("129", (129, 129), 21, (0, 16, 0, 16)), ("161x225", (161, 225), 51, (70, 86, 100, 116)),
              ("512x1024", (512, 1024), 31, (250, 258, 500, 508))]
TINY_SIZE, TINY_SEED = (65, 97), 61


def flip_tag(flip):
    return "flip" if flip else "noflip"


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
    print("  wrote %-40s %7.1f KB" % (name + ".npz", os.path.getsize(path) / 1024))


def run_case(ref, fe, cls, hw, seed, flip, scales):
    x = mg.t(synth.synth_image(1, hw[0], hw[1], seed=seed))
    lab = synth.synth_label(1, hw[0], hw[1], 19, seed=seed)
    with torch.no_grad():
        probs = ref.util.multi_scale_inference(fe, cls, x, mg.t(lab), flip=flip, scales=list(scales))
    pred = probs.max(1)[1]
    return probs, pred, mg.eval_record(ref, probs, pred, lab)


def g_tiny(ref, out):
    fe, cls = mg.build_ref_net(ref, "resnet_tiny")
    fe.eval()
    cls.eval()
    for tag, scales in SCALE_SETS.items():
        for flip in (False, True):
            probs, pred, ev = run_case(ref, fe, cls, TINY_SIZE, TINY_SEED, flip, scales)
            save(out, "g14_tiny_%s_%s" % (tag, flip_tag(flip)), probs=probs.numpy(), pred=pred.numpy().astype(np.uint8),
                 scales=np.array(scales, np.float64), flip=np.array(flip), **ev)


def g_r101(ref, out):
    fe, cls = mg.build_ref_net(ref, "resnet101")
    fe.eval()
    cls.eval()
    for name, hw, seed, crop in R101_CASES:
        for flip in (False, True):
            probs, pred, ev = run_case(ref, fe, cls, hw, seed, flip, SCALE_SETS["s07_10_13"])
            y0, y1, x0, x1 = crop
            save(out, "g14_r101_%s_%s" % (name, flip_tag(flip)), probs_crop=probs.numpy()[0, :, y0:y1, x0:x1], crop=np.array(crop, np.int64),
                 pred=pred.numpy().astype(np.uint8), scales=np.array(SCALE_SETS["s07_10_13"], np.float64), flip=np.array(flip), **ev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--only", choices=("tiny", "r101"), default=None)
    args = ap.parse_args()
    torch.manual_seed(0)
    ref = mg.import_reference()
    if args.only in (None, "tiny"):
        g_tiny(ref, args.out)
    if args.only in (None, "r101"):
        g_r101(ref, args.out)


if __name__ == "__main__":
    main()
