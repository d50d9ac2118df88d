"""Host side of the `aspp` input transform, no GPU: the numpy restatements the kernels follow against PIL itself, the plan sampler, the
GTA5 / Cityscapes datasets on trees written into tmp_path, build_dataset's routing and the C-ABI entry."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _augment_ref as ref
from rnd_semantic_segmentation_amd import _lib
from rnd_semantic_segmentation_amd.host import augment, data, datasets
from rnd_semantic_segmentation_amd.host.config import CfgNode, default_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = ["deeplabv2_r101_src.yaml", "deeplabv2_r101_adv.yaml", "gald_src.yaml", "gald_adv.yaml", "pranet_src_polyp.yaml"]


def make_cfg(**over):
    cfg = CfgNode(default_tree())
    cfg.merge_from_list([x for kv in over.items() for x in (kv[0].replace("__", "."), kv[1])])
    return cfg


# ---- restatements against PIL -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(105, 191, 72, 128), (64, 96, 91, 143), (100, 200, 50, 100), (77, 131, 115, 131), (77, 131, 77, 60), (263, 479, 97, 177)])
def test_bicubic_and_nearest_restatements_equal_pil(shape):
    Image = pytest.importorskip("PIL.Image")
    H, W, oh, ow = shape
    rng = np.random.default_rng(H)
    a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    assert np.array_equal(ref.np_bicubic_resize(a, oh, ow), np.asarray(Image.fromarray(a).resize((ow, oh), Image.BICUBIC)))
    lab = rng.integers(0, 34, (H, W)).astype(np.float32)
    assert np.array_equal(ref.np_nearest(lab, oh, ow), np.asarray(Image.fromarray(lab).resize((ow, oh), Image.NEAREST)))


def test_blend_restatements_equal_pil():
    pytest.importorskip("PIL")
    from PIL import Image
    a = np.random.default_rng(0).integers(0, 256, (97, 131, 3), dtype=np.uint8)
    im = Image.fromarray(a)
    for f in (0.0, 0.5, 0.73, 1.0, 1.31, 1.5):
        for code in (augment.OP_BRIGHTNESS, augment.OP_CONTRAST, augment.OP_SATURATION):
            assert np.array_equal(ref.np_jitter(a, code, f), np.asarray(ref.pil_jitter(im, code, f))), (code, f)


def test_hsv_restatements_equal_pil():
    """A fixed subsample of the 2^24 colours plus the full grey axis, every pure-hue ramp (the six sector boundaries lie on them) and the
    colours next to the boundaries; both directions."""
    pytest.importorskip("PIL")
    from PIL import Image
    rng = np.random.default_rng(1)
    v = np.arange(256, dtype=np.uint8)
    z, f = np.zeros(256, np.uint8), np.full(256, 255, np.uint8)
    ramps = [np.stack(c, -1) for c in ((v, v, v), (f, v, z), (v, f, z), (z, f, v), (z, v, f), (v, z, f), (f, z, v), (f, v, v), (v, f, v), (v, v, f))]
    near = np.stack([np.stack(c, -1) for c in ((f, f - 1, z), (f - 1, f, z), (z, f, f - 1), (z, f - 1, f), (f - 1, z, f), (f, z, f - 1))])
    colours = np.concatenate([np.concatenate(ramps), near.reshape(-1, 3), rng.integers(0, 256, (1 << 20, 3), dtype=np.uint8)])
    a = colours[:(len(colours) // 1024) * 1024].reshape(-1, 1024, 3)
    assert np.array_equal(ref.np_rgb2hsv(a), np.asarray(Image.fromarray(a).convert("HSV")))
    assert np.array_equal(ref.np_hsv2rgb(a), np.asarray(Image.fromarray(a, "HSV").convert("RGB")))
    for amount in (-0.2, -0.03, 0.004, 0.11, 0.5):
        assert np.array_equal(ref.np_jitter(a, augment.OP_HUE, amount), np.asarray(ref.pil_jitter(Image.fromarray(a), augment.OP_HUE, amount))), amount


def test_fixtures_are_what_pil_gives_today():
    """The committed fixtures against the installed PIL (skipped without it): a fixture that drifted from the oracle would test nothing."""
    pytest.importorskip("PIL")
    for name in ref.FIXTURES:
        for i, (image, label, plan, exp_u8, exp_lab) in enumerate(ref.load_fixture(name)):
            got_u8, got_lab = ref.run_plan_pil(image, label, plan)
            assert np.array_equal(got_u8, exp_u8) and np.array_equal(got_lab, exp_lab), (name, i)
            rest_u8, rest_lab = ref.run_plan_numpy(image, label, plan)
            assert np.array_equal(rest_u8, exp_u8) and np.array_equal(rest_lab, exp_lab), (name, i)
            assert np.array_equal(ref.grey_levels(ref.to_tensor_normalize(exp_u8, plan), plan), exp_u8)


def test_bgr255_product_is_exact_for_all_levels():
    u = torch.arange(256, dtype=torch.float32)
    assert torch.equal(u.div(255) * 255, u)


# ---- plans -----------------------------------------------------------------------------------------------------------------------------------
def test_plan_sampling_stays_inside_the_reference_ranges():
    spec = augment.AugmentSpec((100, 180), True, jitter=(0.5, 0.4, 1.5, 0.2), scales=(0.5, 1.5), flip_prob=0.5)
    orders, flips, padded, cropped = set(), set(), 0, 0
    for seed in range(400):
        p = augment.sample_plan(spec, 150, 280, seed=seed, epoch=seed % 3, index=seed * 7)
        f = dict(p.ops)
        assert set(f) == set(augment.OP_NAMES)
        assert 0.5 <= f[augment.OP_BRIGHTNESS] <= 1.5 and 0.6 <= f[augment.OP_CONTRAST] <= 1.4 and 0.0 <= f[augment.OP_SATURATION] <= 2.5 and -0.2 <= f[augment.OP_HUE] <= 0.2
        orders.add(tuple(c for c, _ in p.ops))
        flips.add(p.flip)
        assert int(150 * 0.5) <= p.sh <= int(150 * 1.5) and int(280 * 0.5) <= p.sw <= int(280 * 1.5)
        assert p.pad_y == max(100 - p.sh, 0) and p.pad_x == max(180 - p.sw, 0)                 # the whole deficit on BOTH sides
        assert 0 <= p.crop_y <= p.sh + 2 * p.pad_y - 100 and 0 <= p.crop_x <= p.sw + 2 * p.pad_x - 180
        assert (p.out_h, p.out_w, p.lab_h, p.lab_w, p.lab_sh, p.lab_sw) == (100, 180, 100, 180, p.sh, p.sw)
        padded += p.pad_x > 0
        cropped += p.crop_x > 0
    assert len(orders) > 12 and flips == {0, 1} and padded > 20 and cropped > 200


def test_disabled_ops_are_absent_and_unit_scales_give_the_resize_plan():
    spec = augment.AugmentSpec((72, 128), True, jitter=(0.0, 0.3, 0.0, 0.1))
    for seed in range(50):
        p = augment.sample_plan(spec, 105, 191, seed=seed)
        assert {c for c, _ in p.ops} == {augment.OP_CONTRAST, augment.OP_HUE}
        assert (p.sh, p.sw, p.pad_y, p.pad_x, p.crop_y, p.crop_x, p.flip) == (72, 128, 0, 0, 0, 0, 0)
    plain = augment.sample_plan(augment.AugmentSpec((72, 128), True), 105, 191)
    assert plain.ops == [] and plain.windows()[:4] == (0, 72, 0, 128)
    test = augment.sample_plan(augment.AugmentSpec((72, 128), False, jitter=(0.5, 0.5, 0.5, 0.2), flip_prob=1.0), 105, 191)
    assert test.ops == [] and test.flip == 0 and (test.lab_h, test.lab_w, test.lab_sh, test.lab_sw) == (105, 191, 105, 191)


def test_plan_depends_on_seed_epoch_index_only():
    spec = augment.AugmentSpec((100, 180), True, jitter=(0.5, 0.5, 0.5, 0.2), scales=(0.5, 1.5), flip_prob=0.5)
    key = lambda p: (p.ops, p.sh, p.sw, p.crop_y, p.crop_x, p.flip)
    a = augment.sample_plan(spec, 150, 280, seed=3, epoch=2, index=17)
    assert key(a) == key(augment.sample_plan(spec, 150, 280, seed=3, epoch=2, index=17))
    assert all(key(a) != key(augment.sample_plan(spec, 150, 280, seed=s, epoch=e, index=i)) for s, e, i in ((4, 2, 17), (3, 3, 17), (3, 2, 18)))


def test_padding_rule_pads_both_sides_and_windows_follow():
    p = augment.Plan(260, 480, [], 78, 144, 22, 36, 7, 19, 0, 100, 180, False, (0, 0, 0), (1, 1, 1))
    assert (p.off_y, p.off_x) == (-15, -17)
    cy0, cy1, cx0, cx1, ry0, ry1, rx0, rx1 = p.windows()
    assert (cy0, cy1, cx0, cx1) == (0, 78, 0, 144) and (ry0, ry1, rx0, rx1) == (0, 260, 0, 480)
    q = augment.Plan(200, 360, [], 300, 540, 0, 0, 83, 211, 1, 100, 180, False, (0, 0, 0), (1, 1, 1))
    cy0, cy1, cx0, cx1, ry0, ry1, rx0, rx1 = q.windows()
    assert (cy0, cy1, cx0, cx1) == (83, 183, 211, 391)
    assert 0 < ry0 < 83 * 200 // 300 and ry1 < 200 and ry1 - ry0 < 80 and 0 < rx0 and rx1 - rx0 < 130      # most of the source is never touched
    with pytest.raises(AssertionError, match="crop outside"):
        augment.Plan(260, 480, [], 78, 144, 22, 36, 23, 0, 0, 100, 180, False, (0, 0, 0), (1, 1, 1))


def test_coefficient_tables_are_normalised_fixed_point():
    for a, b in ((480, 180), (100, 180), (1914, 1280)):
        coef, bound, k = augment.bicubic_tables(a, b)
        assert coef.shape == (k, b) and bound.shape == (b, 2) and coef.dtype == np.int32
        assert np.all(bound[:, 0] >= 0) and np.all(bound[:, 0] + bound[:, 1] <= a) and np.all(bound[:, 1] <= k)
        assert np.all(np.abs(coef.sum(0).astype(np.int64) - (1 << augment.PRECISION_BITS)) <= k)
        assert np.all(coef[np.arange(k)[:, None] >= bound[None, :, 1]] == 0)
        assert np.abs(coef.astype(np.int64)).sum(0).max() * 255 < 2 ** 31                           # the kernels accumulate in int32


# ---- datasets ----------------------------------------------------------------------------------------------------------------------------------
def write_trees(root):
    from PIL import Image
    for fold, n, hw in (("fold_0", 2, (40, 64)), ("fold_1", 3, (40, 64)), ("fold_2", 1, (32, 48))):
        for sub in ("images", "labels"):
            os.makedirs(os.path.join(root, "gta5", fold, sub))
        for i in range(n):
            Image.fromarray(ref.synth_picture(hw[0], hw[1], 100 + i)).save(os.path.join(root, "gta5", fold, "images", "%s_%05d.png" % (fold[-1], i)))
            Image.fromarray(ref.synth_ids(hw[0], hw[1], 100 + i)).save(os.path.join(root, "gta5", fold, "labels", "%s_%05d.png" % (fold[-1], i)))
    for split, cities in (("train", (("aachen", 2), ("bochum", 1))), ("val", (("frankfurt", 2), ("lindau", 1)))):
        for city, n in cities:
            os.makedirs(os.path.join(root, "cityscapes", "leftImg8bit", split, city))
            os.makedirs(os.path.join(root, "cityscapes", "gtFine", split, city))
            for i in range(n):
                stem = "%s_%06d_000019" % (city, i)
                hw = (32, 64) if city != "lindau" else (48, 96)
                Image.fromarray(ref.synth_picture(hw[0], hw[1], 200 + i)).save(os.path.join(root, "cityscapes", "leftImg8bit", split, city, stem + "_leftImg8bit.png"))
                Image.fromarray(ref.synth_ids(hw[0], hw[1], 200 + i)).save(os.path.join(root, "cityscapes", "gtFine", split, city, stem + "_gtFine_labelIds.png"))


def test_datasets_pair_files_select_folds_and_map_labels(tmp_path):
    pytest.importorskip("PIL")
    root = str(tmp_path)
    write_trees(root)
    cfg = make_cfg(DATASETS__DATASET_DIR=root, DATASETS__SOURCE_TRAIN="gta5_train", DATASETS__TARGET_TRAIN="cityscapes_train", DATASETS__TEST="cityscapes_val",
                   DATASETS__CROSS_VAL=1, AUG__NAME="aspp", MODEL__NUM_CLASSES=19)
    src = data.build_dataset(cfg, "train", True)
    assert isinstance(src, datasets.GTA5FoldDataSet) and src.device_transform and len(src) == 3            # folds 0 and 2
    assert [os.path.basename(p) for p in src.image_paths] == ["0_00000.png", "0_00001.png", "2_00000.png"]
    image, ids, name = src[2]
    assert image.dtype == torch.uint8 and tuple(image.shape) == (32, 48, 3) and ids.dtype == torch.uint8 and tuple(ids.shape) == (32, 48) and name == "2_00000"
    assert np.array_equal(image.numpy(), ref.synth_picture(32, 48, 100)) and np.array_equal(ids.numpy(), ref.synth_ids(32, 48, 100))
    val = datasets.DatasetCatalog.get(cfg, "gta5_val", "val", 19, cross_val=1)
    assert [os.path.basename(p) for p in val.image_paths] == ["1_00000.png", "1_00001.png", "1_00002.png"]
    every = datasets.DatasetCatalog.get(cfg, "gta5_train", "train", 19, cross_val=None)                     # str(None) is in no fold's name
    assert len(every) == 6
    tgt = data.build_dataset(cfg, "train", False)
    assert isinstance(tgt, datasets.cityscapesDataSet) and len(tgt) == 3 and tgt.mode == "train"
    test = data.build_dataset(cfg, "test", False)
    assert test.mode == "val" and [tuple(test[i][0].shape[:2]) for i in range(3)] == [(32, 64), (32, 64), (48, 96)]      # `test` reads the split of the name
    assert test[2][2] == "lindau_000000_000019_leftImg8bit" and test._paths(2)[1].endswith("gtFine/val/lindau/lindau_000000_000019_gtFine_labelIds.png")
    assert not test.transform.train and (test.transform.out_h, test.transform.out_w) == (512, 1024)
    # the reference's own path: no transform -> PIL image and a mode-F label with the table applied
    plain = datasets.cityscapesDataSet(os.path.join(root, "cityscapes"), num_classes=19, mode="val")
    im, lb, _ = plain[0]
    ids = ref.synth_ids(32, 64, 200)
    assert im.mode == "RGB" and lb.mode == "F" and np.array_equal(np.asarray(lb), datasets.id_table(datasets.TRAINID_19)[ids].astype(np.float32))
    sixteen = datasets.cityscapesDataSet(os.path.join(root, "cityscapes"), num_classes=16, mode="val")
    t19, t16 = plain.id_table, sixteen.id_table
    assert (t19 != 255).sum() == 19 and (t16 != 255).sum() == 16 and t19[33] == 18 and t16[33] == 15 and t16[22] == 255 and t16[23] == 9 and t19[0] == 255
    assert list(sixteen.trainid2name.values())[9] == "sky" and list(plain.trainid2name.values())[9] == "terrain"
    called = []
    hooked = datasets.GTA5FoldDataSet(cfg, os.path.join(root, "gta5"), mode="train", cross_val=1, transform=lambda a, b: (called.append((a.mode, b.mode)), (1, 2))[1])
    assert hooked[0][:2] == (1, 2) and called == [("RGB", "F")]
    # self-distillation: train ids kept, everything else ignored
    os.makedirs(os.path.join(root, "pseudo"))
    from PIL import Image
    for p in tgt.image_paths:
        Image.fromarray(ref.synth_ids(32, 64, 5)).save(os.path.join(root, "pseudo", os.path.basename(p)))
    sd = datasets.cityscapesSelfDistillDataSet(os.path.join(root, "cityscapes"), os.path.join(root, "pseudo"), num_classes=19, mode="train")
    lb = np.asarray(sd[0][1])
    want = ref.synth_ids(32, 64, 5).astype(np.float32)
    want[want > 18] = 255
    assert np.array_equal(lb, want)


def test_build_dataset_keeps_the_synthetic_data_for_every_shipped_configuration(tmp_path):
    for name in CONFIGS:
        cfg = CfgNode(default_tree())
        cfg.merge_from_file(os.path.join(ROOT, "configs", name))
        assert data.build_collate_fn(cfg) is None
        for mode, is_source in (("train", True), ("train", False), ("test", False)):
            ds = data.build_dataset(cfg, mode, is_source)
            assert isinstance(ds, (data.SyntheticSegmentation, data.SyntheticPolyp)), (name, mode)
    # the new configurations too, until their directory exists
    for name in ("deeplabv2_r101_src_gta5.yaml", "deeplabv2_r101_adv_gta5.yaml"):
        cfg = CfgNode(default_tree())
        cfg.merge_from_file(os.path.join(ROOT, "configs", name))
        cfg.merge_from_list(["DATASETS.DATASET_DIR", str(tmp_path / "nothing")])
        assert isinstance(data.build_dataset(cfg, "train", True), data.SyntheticSegmentation) and data.build_collate_fn(cfg) is None
    pytest.importorskip("PIL")
    write_trees(str(tmp_path))
    cfg.merge_from_list(["DATASETS.DATASET_DIR", str(tmp_path)])
    assert isinstance(data.build_dataset(cfg, "train", True), datasets.GTA5FoldDataSet) and data.build_collate_fn(cfg) is None
    spec = data.build_dataset(cfg, "train", True).transform
    assert (spec.brightness, spec.contrast, spec.saturation, spec.hue) == (0.5, 0.5, 0.5, 0.2) and (spec.out_h, spec.out_w) == (720, 1280)
    assert data.build_dataset(cfg, "train", False).transform.hue == 0.0                                       # ColorJitter: source only
    cfg.merge_from_list(["AUG.NAME", "attn"])
    with pytest.raises(ValueError, match="AUG.NAME"):
        data.build_dataset(cfg, "train", True)


def test_loader_draws_plans_by_dataset_index_and_epoch(tmp_path):
    pytest.importorskip("PIL")
    write_trees(str(tmp_path))
    cfg = make_cfg(DATASETS__DATASET_DIR=str(tmp_path), DATASETS__SOURCE_TRAIN="gta5_train", AUG__NAME="aspp", MODEL__NUM_CLASSES=19,
                   INPUT__INPUT_SCALES_TRAIN=(0.5, 1.5), INPUT__HUE=0.2, INPUT__SOURCE_INPUT_SIZE_TRAIN=(48, 32))
    ds = data.build_dataset(cfg, "train", True)
    loader = datasets.wrap_loader(ds, batch_size=2, shuffle=True, num_workers=40, drop_last=True, pin_memory=True, collate_fn=None)
    assert isinstance(loader, datasets.DeviceAugmentLoader) and loader.num_workers == 16 and len(loader) == 2 and loader.batch_size == 2
    assert loader.dataset is ds and isinstance(loader.sampler, torch.utils.data.RandomSampler)
    key = lambda p: (p.ops, p.sh, p.sw, p.crop_y, p.crop_x)
    a = loader.plans_for([3, 0], [(40, 64), (40, 64)], epoch=0)
    b = loader.plans_for([0], [(40, 64)], epoch=0)
    assert key(a[1]) == key(b[0]) and key(a[0]) != key(a[1])
    assert key(loader.plans_for([0], [(40, 64)], epoch=1)[0]) != key(b[0])
    assert np.array_equal(a[0].label_table, ds.id_table)
    loader.set_start_epoch(4)
    assert loader.epoch == 4
    synthetic = datasets.wrap_loader(data.SyntheticSegmentation(cfg), batch_size=2, num_workers=0)
    assert isinstance(synthetic, torch.utils.data.DataLoader)


def test_dropin_paths_resolve_to_the_datasets():
    from core.datasets.cityscapes import cityscapesDataSet, cityscapesSelfDistillDataSet
    from core.datasets.dataset_path_catalog import DatasetCatalog
    from core.datasets.gta5 import GTA5FoldDataSet
    assert (DatasetCatalog, GTA5FoldDataSet, cityscapesDataSet, cityscapesSelfDistillDataSet) == (
        datasets.DatasetCatalog, datasets.GTA5FoldDataSet, datasets.cityscapesDataSet, datasets.cityscapesSelfDistillDataSet)


# ---- C-ABI ---------------------------------------------------------------------------------------------------------------------------------------
def test_augment_entry_is_declared_bound_and_validates_without_a_gpu():
    import __graft_entry__ as entry
    entry.build()
    src = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    m = re.search(r"\bint\s+mi_augment_batch\s*\(([^;{]*)\)\s*;", src)
    assert m and m.group(1).count(",") + 1 == len(_lib.SIGNATURES["mi_augment_batch"][1]) == 10
    assert "augment.hip" in entry.SOURCES
    fields = re.search(r"typedef struct MiAugSample \{(.*?)\} MiAugSample;", src, flags=re.S).group(1)
    declared = [n.strip().split("[")[0].lstrip("*") for line in fields.split(";") if line.strip() for n in line.strip().split(None, 1)[1].replace("uint8_t*", "").replace("int32_t*", "").replace("long long", "").split(",")]
    assert declared == [f[0] for f in _lib.MiAugSample._fields_]
    L = _lib.lib()
    assert L.mi_augment_batch(None, None, 1, 8, 8, 0, 0, None, None, None) == -22 and b"null operand" in L.mi_last_error()
    rec = (_lib.MiAugSample * 1)()
    one = ctypes.c_void_p(64)
    args = (one, ctypes.cast(rec, ctypes.c_void_p), 1, 8, 8, 0, 0, one, None, None)
    assert L.mi_augment_batch(*args) == -22 and b"sample 0: image" in L.mi_last_error()
    rec[0].img, rec[0].H, rec[0].W, rec[0].sh, rec[0].sw, rec[0].n_ops = 64, 16, 16, 8, 8, 5
    assert L.mi_augment_batch(*args) == -22 and b"n_ops 5" in L.mi_last_error()
    rec[0].n_ops = 0
    assert L.mi_augment_batch(*args) == -22 and b"tables exactly when its size changes" in L.mi_last_error()
