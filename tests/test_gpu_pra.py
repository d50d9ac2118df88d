"""csrc/augment_pra.hip (mi_augment_pra_batch) against the PIL oracle of tests/_pra_ref.py, through the fixtures tests/golden/g18_pra_*.npz
(tools/make_pra_golden.py): every stage up to the uint8 image is integer or table arithmetic that the plan determines completely, so the
requirement is equality - mask, grey levels and the float32 bits - not a tolerance.  Then the Kvasir loader end to end through the unchanged
scripts."""
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import _pra_ref as ref
from rnd_semantic_segmentation_amd.host import augment, pra_augment as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fixtures():
    return {name: ref.load_fixture(name) for name in ref.FIXTURES}


def run_samples(samples):
    aug = augment.DeviceAugmenter("cuda")
    img, mask = aug([s[0] for s in samples], [s[1] for s in samples], [s[2] for s in samples])
    torch.cuda.synchronize()
    return img.cpu(), mask.cpu()


def describe(p):
    return "%dx%d sym %d crop %d window [%d,+%d)x[%d,+%d) -> %dx%d hsv %d (hue %d, s %+g, v %+g) bc %d (%g, %+g)" % (
        p.H, p.W, p.sym, p.crop, p.y0, p.wh, p.x0, p.ww, p.out_h, p.out_w, p.hsv, p.hue_shift, p.sat_shift, p.val_shift, p.bc, p.alpha, p.beta)


@pytest.mark.parametrize("name", ref.FIXTURES)
def test_kernels_equal_the_pil_oracle_sample_by_sample(name, fixtures):
    """Every sample of the fixture run alone: mask equal in every element, image equal in every element once mapped back to grey levels,
    float32 output equal to ToTensor + Normalize (torch, CPU) of the oracle's uint8 image bit for bit."""
    for i, s in enumerate(fixtures[name]):
        image, mask, plan, exp_u8, exp_mask = s
        got_img, got_mask = run_samples([s])
        what = "%s[%d] %s" % (name, i, describe(plan))
        assert got_mask.shape == (1,) + exp_mask.shape and got_img.shape == (1, 3, plan.out_h, plan.out_w), what
        nmask = int((got_mask[0].numpy() != exp_mask).sum())
        levels = ref.grey_levels(got_img[0], plan)
        nlev = int((levels != exp_u8.astype(np.int64)).sum())
        want = ref.to_tensor_normalize(exp_u8, plan)
        nbits = int((got_img[0].view(torch.int32) != want.view(torch.int32)).sum())
        print("%s: mask differs in %d, grey levels in %d (max %d), float32 bits in %d of %d" % (
            what, nmask, nlev, int(np.abs(levels - exp_u8.astype(np.int64)).max()), nbits, want.numel()))
        assert nmask == 0, what
        assert nlev == 0, what
        assert nbits == 0, what


@pytest.mark.parametrize("name", ref.FIXTURES)
def test_batch_gives_the_bits_of_each_sample_alone_and_is_repeatable(name, fixtures):
    samples = fixtures[name]
    img, mask = run_samples(samples)
    img2, mask2 = run_samples(samples)
    assert torch.equal(img.view(torch.int32), img2.view(torch.int32)) and torch.equal(mask, mask2)
    for i, s in enumerate(samples):
        one_img, one_mask = run_samples([s])
        assert torch.equal(img[i].view(torch.int32), one_img[0].view(torch.int32)), (name, i)
        assert torch.equal(mask[i], one_mask[0]), (name, i)


def test_fixtures_cover_what_the_issue_lists(fixtures):
    plans = [s[2] for n in ref.FIXTURES for s in fixtures[n]]
    assert {p.sym for p in plans} == set(range(8))
    rand = [p for p in plans if p.crop == P.CROP_RANDOM]
    assert any(p.y0 == 0 and p.x0 == 0 for p in rand)                                                            # u = 0
    assert any(p.y0 == p.frame[0] - 220 - 1 and p.x0 == p.frame[1] - 220 - 1 for p in rand)                      # the largest offset int((n - 220) * u), u < 1
    assert any(p.sym & 4 for p in rand) and any(not p.sym & 4 for p in rand)
    assert any(p.crop == P.CROP_CENTER and (p.y0, p.x0) == ((p.frame[0] - 220) // 2, (p.frame[1] - 220) // 2) for p in plans)
    assert any(p.crop == P.CROP_TOO_SMALL and min(p.frame) < 220 and (p.wh, p.ww) == p.frame for p in plans)
    assert any(p.crop == P.CROP_NOT_DRAWN and min(p.frame) >= 220 and (p.wh, p.ww) == p.frame for p in plans)
    hsv = [p for p in plans if p.hsv]
    assert any(not p.hsv for p in plans) and any(p.hue_shift < 128 for p in hsv) and any(p.hue_shift >= 128 for p in hsv)      # wraps upward / downward
    for table in ("lut_s", "lut_v"):
        assert any(getattr(p, table)[1] == 0 for p in hsv) and any(getattr(p, table)[254] == 255 for p in hsv)                # clipping at 0 / at 255
    bc = [p for p in plans if p.bc]
    assert any(not p.bc for p in plans) and any(p.alpha < 1 for p in bc) and any(p.alpha > 1 for p in bc)
    test = [s[2] for s in fixtures["g18_pra_test"]]
    assert all((p.sym, p.crop, p.hsv, p.bc) == (0, 0, 0, 0) and (p.wh, p.ww) == (p.H, p.W) for p in test) and test[0].out_h != test[0].out_w
    assert any(len({(s[2].H, s[2].W) for s in fixtures[n]}) > 1 for n in ref.FIXTURES)                             # a batch of mixed sizes
    shapes = {(p.H, p.W, p.out_h) for p in plans if p.crop in (P.CROP_NOT_DRAWN, P.CROP_TOO_SMALL) and p.out_h == p.out_w}
    assert {(236, 251, 96), (97, 130, 128), (96, 301, 96), (531, 617, 64)} <= shapes
    assert augment.resample_tables(251, 96, "bilinear")[2] == 7 and augment.resample_tables(617, 64, "bilinear")[2] == 21 and (130 * 3) % 4 != 0
    assert any((p.H, p.W) == (96, 301) and p.wh == p.out_h and p.ww != p.out_w for p in plans)                    # the vertical pass skipped
    assert any((p.H, p.W) == (96, 301) and p.ww == p.out_w and p.wh != p.out_h for p in plans)                    # the horizontal pass skipped
    masks = [s[1] for n in ref.FIXTURES for s in fixtures[n]]
    assert all({127, 128} <= set(np.unique(m).tolist()) and m.min() < 127 and m.max() > 128 for m in masks)


def test_bad_records_are_refused_before_any_launch(fixtures):
    from rnd_semantic_segmentation_amd import _lib, kernels
    image, mask, plan, _, _ = fixtures["g18_pra_symmetry"][4]                   # transposed, 220 window at y0 = 30 of the 251 x 236 frame
    aug = augment.DeviceAugmenter("cuda")
    with pytest.raises(ValueError, match="uint8"):
        aug([image[:-1]], [mask], [plan])
    bad = P.PraPlan.from_arrays(plan.to_arrays())
    bad.x0 = 17                                                                  # 17 + 220 > 236
    with pytest.raises(_lib.MiError, match="outside the transformed frame"):
        aug([image], [mask], [bad])
    # hand-made records: a null image, then a table of the wrong taps
    dev = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    host = torch.zeros(1 << 16, dtype=torch.uint8)
    out = torch.full((1, 3, 8, 8), 7.0, device="cuda")
    r = _lib.MiPraSample.from_buffer(host.numpy())
    r.H, r.W, r.wh, r.ww, r.wstride, r.tstride = 16, 16, 16, 16, 48, 24
    for k in range(3):
        r.std[k] = 1.0
    with pytest.raises(_lib.MiError, match="sample 0: image"):
        kernels.augment_pra_batch(dev, host, 1, out)
    base = dev.data_ptr()
    r.img, r.win, r.tmp = base + 4096, base + 8192, base + 12288
    r.hcoef = r.hbound = r.vcoef = r.vbound = base + 16384
    r.hk, r.vk = 5, 3                                                            # 16 -> 8 has 2 * ceil(2) + 1 = 5 taps
    with pytest.raises(_lib.MiError, match="taps"):
        kernels.augment_pra_batch(dev, host, 1, out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                              # nothing was launched


# ---- end to end: the unchanged scripts on a Kvasir tree written with PIL --------------------------------------------------------------------------
def run(args, env_extra):
    env = dict(os.environ, **env_extra)
    return subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)


def write_tree(root):
    from PIL import Image
    for fold, n, hw in (("fold_0", 2, (120, 200)), ("fold_1", 3, (236, 251)), ("fold_2", 3, (120, 200))):
        for sub in ("images", "masks"):
            os.makedirs(os.path.join(root, "kvasir", fold, sub))
        for i in range(n):
            Image.fromarray(ref.synth_picture(hw[0], hw[1], 300 + i)).save(os.path.join(root, "kvasir", fold, "images", "%s%03d.png" % (fold[-1], i)))
            Image.fromarray(ref.synth_mask(hw[0], hw[1], 300 + i)).save(os.path.join(root, "kvasir", fold, "masks", "%s%03d.png" % (fold[-1], i)))


def test_train_src_on_a_kvasir_tree_then_test_py_on_the_held_out_fold(tmp_path):
    pytest.importorskip("PIL")
    from PIL import Image
    data_dir = str(tmp_path / "data")
    write_tree(data_dir)
    out = str(tmp_path / "pranet") + "/"
    t0 = time.perf_counter()
    common = ["-cfg", "configs/pranet_src_kvasir.yaml", "DATASETS.DATASET_DIR", data_dir, "OUTPUT_DIR", out]
    r = run(["train_src.py", "--model", "pranet"] + common + ["SOLVER.EPOCHS", "2", "SOLVER.CHECKPOINT_PERIOD", "1", "SOLVER.BATCH_SIZE", "2", "INPUT.TRAINSIZE", "96"], {})
    assert r.returncode == 0, r.stderr[-3000:]
    log = r.stderr + r.stdout
    losses = [float(v) for v in re.findall(r"lateral-\d: (\S+?),", log)]
    assert len(losses) >= 8 and all(np.isfinite(v) and v > 0 for v in losses), losses                              # folds 1 and 2: 6 pictures, 3 batches of mixed sizes
    ck = torch.load(os.path.join(out, "PraNet-2.pth"), map_location="cpu")
    assert set(ck) == {"epoch", "model", "optimizer"} and ck["epoch"] == 2 and len(ck["model"]) == 922
    assert int(ck["model"]["resnet.bn1.num_batches_tracked"]) == 18                                                 # 2 epochs x 3 batches x 3 passes
    assert set(ck["optimizer"]["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and float(ck["optimizer"]["state"][0]["step"]) == 18
    r = run(["test.py", "-c", "renders/kvasir.json"] + common + ["resume",os.path.join(out, "PraNet-2.pth"), "INPUT.INPUT_SIZE_TEST", "(96, 96)"], {})
    assert r.returncode == 0, r.stderr[-3000:]
    assert "Micro metric, val result: mIoU/mF1" in r.stderr + r.stdout
    print("train_src.py + test.py: %.1f s" % (time.perf_counter() - t0))
    # the batches the loader yields are the oracle's on the decoded PNGs with the loader's own plans
    from rnd_semantic_segmentation_amd.host import data, datasets
    from rnd_semantic_segmentation_amd.host.config import CfgNode, default_tree
    cfg = CfgNode(default_tree())
    cfg.merge_from_file(os.path.join(ROOT, "configs", "pranet_src_kvasir.yaml"))
    cfg.merge_from_list(["DATASETS.DATASET_DIR", data_dir, "INPUT.TRAINSIZE", 96, "INPUT.INPUT_SIZE_TEST", (96, 80)])
    for mode, count in (("train", 6), ("test", 2)):
        ds = data.build_dataset(cfg, mode, mode == "train")
        assert isinstance(ds, datasets.KvasirFoldDataset) and len(ds) == count
        # (decoded in this process: with two decode workers this check took 13 s run alone and 95 s behind the whole GPU suite, whose process they are forked from)
        loader = datasets.wrap_loader(ds, batch_size=2, shuffle=False, num_workers=0, drop_last=True, pin_memory=True, collate_fn=None)
        loader.set_start_epoch(3)
        seen = 0
        for b, (img, mask, names) in enumerate(loader):
            torch.cuda.synchronize()
            indices = [2 * b, 2 * b + 1]
            assert names == [os.path.basename(ds.image_paths[i])[:-4] for i in indices]
            decoded = [(np.array(Image.open(ds._paths(i)[0]).convert("RGB")), np.array(Image.open(ds._paths(i)[1]).convert("L"))) for i in indices]
            plans = loader.plans_for(indices, [d[0].shape[:2] for d in decoded], epoch=3)
            assert tuple(mask.shape) == (2, plans[0].out_h, plans[0].out_w) and (plans[0].out_h, plans[0].out_w) == ((96, 96) if mode == "train" else (80, 96))
            for j, ((im, mk), plan) in enumerate(zip(decoded, plans)):
                exp_u8, exp_mask = ref.run_plan_pil(im, mk, plan)
                assert torch.equal(img[j].cpu().view(torch.int32), ref.to_tensor_normalize(exp_u8, plan).view(torch.int32)), (mode, b, j, describe(plan))
                assert np.array_equal(mask[j].cpu().numpy(), exp_mask), (mode, b, j, describe(plan))
                seen += 1
        assert seen == count
