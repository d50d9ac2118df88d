"""csrc/augment.hip (mi_augment_batch) against the PIL oracle of tests/_augment_ref.py, through the fixtures tests/golden/g15_*.npz
(tools/make_augment_golden.py): the uint8 stages are integer arithmetic that the plan determines completely, so the requirement is
equality - label, grey levels and the float32 bits - not a tolerance.  Then the loader end to end through the unchanged scripts."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _augment_ref as ref
from rnd_semantic_segmentation_amd.host import augment

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_samples(samples):
    aug = augment.DeviceAugmenter("cuda")
    img, lab = aug([s[0] for s in samples], [s[1] for s in samples], [s[2] for s in samples])
    torch.cuda.synchronize()
    return img.cpu(), lab.cpu()


def describe(plan):
    ops = ",".join("%s=%g" % (augment.OP_NAMES[c], f) for c, f in plan.ops) or "no jitter"
    return "%dx%d -> %dx%d pad (%d,%d) crop (%d,%d) flip %d bgr255 %d [%s]" % (plan.H, plan.W, plan.sh, plan.sw, plan.pad_y, plan.pad_x, plan.crop_y,
                                                                            plan.crop_x, plan.flip, plan.to_bgr255, ops)


@pytest.mark.parametrize("name", ref.FIXTURES)
def test_kernels_equal_the_pil_oracle_sample_by_sample(name):
    """Every sample of the fixture run alone: label equal in every element, image equal in every element once mapped back to grey levels,
    float32 output equal to ToTensor + Normalize (torch, CPU) of the oracle's uint8 image bit for bit."""
    for i, s in enumerate(ref.load_fixture(name)):
        image, label, plan, exp_u8, exp_lab = s
        got_img, got_lab = run_samples([s])
        what = "%s[%d] %s" % (name, i, describe(plan))
        assert got_lab.shape == (1,) + exp_lab.shape and got_img.shape == (1, 3, plan.out_h, plan.out_w), what
        nlab = int((got_lab[0].numpy() != exp_lab).sum())
        levels = ref.grey_levels(got_img[0], plan)
        nlev = int((levels != exp_u8.astype(np.int64)).sum())
        want = ref.to_tensor_normalize(exp_u8, plan)
        nbits = int((got_img[0].view(torch.int32) != want.view(torch.int32)).sum())
        print("%s: label differs in %d, grey levels in %d (max %d), float32 bits in %d of %d" % (
            what, nlab, nlev, int(np.abs(levels - exp_u8.astype(np.int64)).max()), nbits, want.numel()))
        assert nlab == 0, what
        assert nlev == 0, what
        assert nbits == 0, what


def test_fixtures_cover_what_the_issue_lists():
    plans = [s[2] for n in ref.FIXTURES for s in ref.load_fixture(n)]
    single = {(p.ops[0][0], p.ops[0][1] > (0 if p.ops[0][0] == augment.OP_HUE else 1)) for p in plans if len(p.ops) == 1}
    assert {(c, up) for c in augment.OP_NAMES for up in (False, True)} <= single                      # each op alone, below and above
    assert len({tuple(c for c, _ in p.ops) for p in plans if len(p.ops) == 4}) >= 2                    # all four, two orders
    assert any(p.sh < p.H and p.sw < p.W for p in plans) and any(p.sh > p.H and p.sw > p.W for p in plans)
    assert any(p.sh == p.H and p.sw != p.W for p in plans) and any(p.sw == p.W and p.sh != p.H for p in plans)
    assert any(p.pad_y > 0 and p.pad_x > 0 for p in plans) and any(p.sh > p.out_h and p.crop_y > 0 and p.crop_x > 0 for p in plans)
    assert {p.flip for p in plans} == {0, 1} and {p.to_bgr255 for p in plans} == {0, 1}
    assert any((p.lab_h, p.lab_w) == (p.H, p.W) != (p.out_h, p.out_w) for p in plans)                 # test mode: label untouched
    assert any(len({(s[2].H, s[2].W) for s in ref.load_fixture(n)}) > 1 for n in ref.FIXTURES)        # a batch of different sizes


@pytest.mark.parametrize("name", ref.FIXTURES)
def test_batch_gives_the_bits_of_each_sample_alone_and_is_repeatable(name):
    samples = ref.load_fixture(name)
    img, lab = run_samples(samples)
    img2, lab2 = run_samples(samples)
    assert torch.equal(img.view(torch.int32), img2.view(torch.int32)) and torch.equal(lab, lab2)
    for i, s in enumerate(samples):
        one_img, one_lab = run_samples([s])
        assert torch.equal(img[i].view(torch.int32), one_img[0].view(torch.int32)), (name, i)
        assert torch.equal(lab[i], one_lab[0]), (name, i)


def test_bad_records_are_refused_before_any_launch():
    from rnd_semantic_segmentation_amd import _lib
    image, label, plan, _, _ = ref.load_fixture("g15_geometry")[0]
    aug = augment.DeviceAugmenter("cuda")
    with pytest.raises(ValueError, match="uint8"):
        aug([image[:-1]], [label], [plan])
    bad = augment.Plan.from_arrays(plan.to_arrays())
    bad.windows = lambda: (0, plan.sh, 0, plan.sw + 4, 0, plan.H, 0, plan.W)          # a window wider than the resampled image
    with pytest.raises(_lib.MiError, match="window"):
        aug([image], [label], [bad])


# ---- end to end: the unchanged scripts on trees written with PIL ---------------------------------------------------------------------------
def run(args, env_extra):
    env = dict(os.environ, **env_extra)
    return subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)


def write_trees(root):
    from PIL import Image
    for fold, n, hw in (("fold_0", 2, (120, 200)), ("fold_1", 5, (120, 200)), ("fold_2", 3, (96, 168))):
        for sub in ("images", "labels"):
            os.makedirs(os.path.join(root, "gta5", fold, sub))
        for i in range(n):
            Image.fromarray(ref.synth_picture(hw[0], hw[1], 100 + i)).save(os.path.join(root, "gta5", fold, "images", "%05d.png" % i))
            Image.fromarray(ref.synth_ids(hw[0], hw[1], 100 + i)).save(os.path.join(root, "gta5", fold, "labels", "%05d.png" % i))
    for city, n in (("aachen", 2), ("bochum", 1)):
        os.makedirs(os.path.join(root, "cityscapes", "leftImg8bit", "val", city))
        os.makedirs(os.path.join(root, "cityscapes", "gtFine", "val", city))
        for i in range(n):
            stem = "%s_%06d_000019" % (city, i)
            Image.fromarray(ref.synth_picture(128, 256, 200 + i)).save(os.path.join(root, "cityscapes", "leftImg8bit", "val", city, stem + "_leftImg8bit.png"))
            Image.fromarray(ref.synth_ids(128, 256, 200 + i)).save(os.path.join(root, "cityscapes", "gtFine", "val", city, stem + "_gtFine_labelIds.png"))


def test_train_src_on_a_gta5_tree_then_test_py_on_a_cityscapes_tree(tmp_path):
    pytest.importorskip("PIL")
    from rnd_semantic_segmentation_amd.host import modules, synth
    data = str(tmp_path / "data")
    write_trees(data)
    out = str(tmp_path / "run")
    fe = modules.resnet_feature_extractor("resnet101", freeze_bn=True, pretrained_backbone=False)
    weights = str(tmp_path / "r101_formula.pth")
    torch.save({k: torch.from_numpy(synth.formula_tensor("backbone." + k, v.shape)) for k, v in fe.backbone.state_dict().items()}, weights)
    common = ["-cfg", "configs/deeplabv2_r101_adv_gta5.yaml", "DATASETS.DATASET_DIR", data, "DATASETS.CROSS_VAL", "0", "OUTPUT_DIR", out]
    r = run(["train_src.py"] + common + ["SOLVER.EPOCHS", "1", "MODEL.WEIGHTS", weights, "SOLVER.BATCH_SIZE", "2", "INPUT.SOURCE_INPUT_SIZE_TRAIN", "(161, 129)",
                                         "INPUT.INPUT_SCALES_TRAIN", "(0.8, 1.5)", "INPUT.HORIZONTAL_FLIP_PROB_TRAIN", "0.5"], {})
    assert r.returncode == 0, r.stderr[-3000:]
    chart = json.load(open(os.path.join(out, "aspp_chart_params.json")))
    assert len(chart["loss"]) == 4 and all(np.isfinite(v) and 0 < v < 10 for v in chart["loss"])      # folds 1 and 2: 8 images, batches of 2 of mixed sizes
    r = run(["test.py"] + common + ["resume", os.path.join(out, "Aspp-1.pth"), "INPUT.INPUT_SIZE_TEST", "(193, 97)"], {})
    assert r.returncode == 0, r.stderr[-3000:]
    cm = json.load(open(os.path.join(out, "aspp_confusion_matrix.json")))
    assert len(cm["cmt"]) == 19 and sum(map(sum, cm["cmt"])) > 0
    # every pixel of the three 128x256 labels whose id is in the 19-class table was scored (the label keeps its own size in test mode)
    from rnd_semantic_segmentation_amd.host import datasets
    table = datasets.id_table(datasets.TRAINID_19)
    valid = sum(int((table[ref.synth_ids(128, 256, 200 + i)] != 255).sum()) for i in (0, 1, 0))
    assert sum(map(sum, cm["cmt"])) == valid
