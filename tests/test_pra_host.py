"""Host side of the `pra` input transform, no GPU: the generalised resampling tables against PIL's BILINEAR, the composed symmetry, the
colour tables, the plan sampler, the Kvasir datasets on a tree written into tmp_path, build_dataset's routing and the C-ABI entry."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _pra_ref as ref
from rnd_semantic_segmentation_amd import _lib
from rnd_semantic_segmentation_amd.host import augment, data, datasets, pra_augment as P
from rnd_semantic_segmentation_amd.host.config import CfgNode, default_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_cfg(**over):
    cfg = CfgNode(default_tree())
    cfg.merge_from_list([x for kv in over.items() for x in (kv[0].replace("__", "."), kv[1])])
    return cfg


# ---- tables ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(220, 220, 352), (300, 260, 352), (531, 617, 352), (1070, 1350, 352), (97, 130, 64), (220, 352, 352)])
def test_triangle_tables_through_a_numpy_two_pass_equal_pil_bilinear(shape):
    Image = pytest.importorskip("PIL.Image")
    H, W, S = shape
    a = np.random.default_rng(H).integers(0, 256, (H, W, 3), dtype=np.uint8)
    assert np.array_equal(ref.np_resize(a, S, S), np.asarray(Image.fromarray(a).resize((S, S), Image.BILINEAR)))


def test_bicubic_tables_are_unchanged_by_the_generalisation():
    """Against the formula as it stood before resample_tables took the filter, restated here."""
    def before(in_size, out_size):
        import math
        scale = in_size / out_size
        fs = max(scale, 1.0)
        support = 2.0 * fs
        k = int(math.ceil(support)) * 2 + 1
        center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
        x0 = np.maximum((center - support + 0.5).astype(np.int64), 0)
        n = np.minimum((center + support + 0.5).astype(np.int64), in_size) - x0
        x = np.abs((np.arange(k, dtype=np.float64)[:, None] + x0[None, :] - center[None, :] + 0.5) * (1.0 / fs))
        w = np.where(x < 1.0, (1.5 * x - 2.5) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * -0.5, 0.0))
        w = np.where(np.arange(k)[:, None] < n[None, :], w, 0.0)
        total = np.zeros(out_size, np.float64)
        for t in range(k):
            total = total + w[t]
        w = np.where(total[None, :] != 0.0, w / np.where(total == 0.0, 1.0, total)[None, :], w)
        return np.where(w < 0, -0.5 + w * (1 << 22), 0.5 + w * (1 << 22)).astype(np.int64), np.stack([x0, n], 1), k
    for a, b in ((480, 180), (100, 180), (1914, 1280), (260, 100), (97, 97)):
        coef, bound, k = augment.bicubic_tables(a, b)
        c0, b0, k0 = before(a, b)
        assert k == k0 and np.array_equal(coef, c0) and np.array_equal(bound, b0)
        assert augment.resample_tables(a, b, "bicubic")[0] is coef
    coef, bound, k = augment.resample_tables(617, 64, "bilinear")
    assert k == 21 and coef.shape == (21, 64) and augment.resample_tables(251, 96, "bilinear")[2] == 7 and augment.resample_tables(130, 128, "bilinear")[2] == 5
    assert np.abs(coef.astype(np.int64)).sum(0).max() * 255 < 2 ** 31


@pytest.mark.parametrize("sizes", [(251, 96), (236, 96), (130, 128), (97, 128), (617, 64), (531, 64), (220, 352), (301, 96), (1920, 352), (5, 64)])
def test_nearest_table_is_pils(sizes):
    Image = pytest.importorskip("PIL.Image")
    n_in, n_out = sizes
    row = np.arange(n_in, dtype=np.int32).reshape(1, n_in)
    assert np.array_equal(np.asarray(Image.fromarray(row).resize((n_out, 1), Image.NEAREST))[0], P.nearest_table(n_in, n_out))        # int32 -> mode I


def test_composed_symmetry_equals_the_three_numpy_operations_in_sequence():
    a = np.arange(12).reshape(3, 4)
    seen = set()
    for k in range(4):
        for d in (None, -1, 0, 1):
            for t in (False, True):
                x = np.rot90(a, k)
                if d is not None:
                    x = {0: x[::-1], 1: x[:, ::-1], -1: x[::-1, ::-1]}[d]
                if t:
                    x = x.T
                sym = P.compose_symmetry(k, d, t)
                seen.add(sym)
                assert np.array_equal(x, P.apply_symmetry(a, sym)), (k, d, t)
    assert seen == set(range(8))
    Image = pytest.importorskip("PIL.Image")
    u8 = a.astype(np.uint8)
    for sym in range(8):                                         # the oracle's table of Image.transpose methods says the same
        op = ref.pil_symmetry(sym)
        im = Image.fromarray(u8)
        assert np.array_equal(np.asarray(im if op is None else im.transpose(op)), P.apply_symmetry(u8, sym))


def test_colour_tables_equal_their_formulas_at_both_clipping_ends():
    for s in (-30.0, -0.4, 0.0, 17.3, 30.0):
        t = P.shift_table(s)
        want = [min(max(int(np.float32(i) + np.float32(s)), 0), 255) for i in range(256)]
        assert t.dtype == np.uint8 and t.tolist() == want
    assert P.shift_table(-30.0)[:31].tolist() == [0] * 31 and P.shift_table(-30.0)[31] == 1 and P.shift_table(30.0)[225:].tolist() == [255] * 31
    for alpha, beta in ((0.8, -0.2), (1.2, 0.2), (1.0, 0.0), (1.13, 0.07)):
        t = P.brightness_contrast_table(alpha, beta)
        want = [min(max(int(np.float32(i) * np.float32(alpha) + np.float32(beta * 255.0)), 0), 255) for i in range(256)]
        assert t.tolist() == want
    assert P.brightness_contrast_table(0.8, -0.2)[:64].max() == 0 and P.brightness_contrast_table(1.2, 0.2)[-64:].min() == 255
    assert np.array_equal(P.brightness_contrast_table(1.0, 0.0), np.arange(256))
    assert [P.hue_shift_of(s) for s in (20.0, -20.0, 0.0, -0.3, 7.0)] == [28, 228, 0, 0, 10]
    assert P.MASK_TABLE[127] == 0 and P.MASK_TABLE[128] == 1 and set(P.MASK_TABLE.tolist()) == {0, 1}


# ---- plans -------------------------------------------------------------------------------------------------------------------------------------------
def key(p):
    return tuple(p.to_arrays()["geom"].tolist()) + tuple(p.to_arrays()["colour"].tolist())


def test_plan_round_trips_and_depends_on_seed_epoch_index_only():
    spec = P.PraSpec((96, 96), True)
    a = P.sample_pra_plan(spec, 236, 251, seed=3, epoch=2, index=17)
    b = P.PraPlan.from_arrays(a.to_arrays())
    assert key(a) == key(b) and all(np.array_equal(getattr(a, t), getattr(b, t)) for t in ("lut_s", "lut_v", "lut_bc", "mask_table", "mean", "std"))
    assert key(a) == key(P.sample_pra_plan(spec, 236, 251, seed=3, epoch=2, index=17))
    assert P.draw_pra(3, 2, 17) == P.draw_pra(3, 2, 17)
    assert all(P.draw_pra(3, 2, 17) != P.draw_pra(s, e, i) for s, e, i in ((4, 2, 17), (3, 3, 17), (3, 2, 18)))
    t = P.sample_pra_plan(P.PraSpec((64, 112), False), 236, 251, seed=3, epoch=2, index=17)
    assert (t.sym, t.crop, t.y0, t.x0, t.wh, t.ww, t.out_h, t.out_w, t.hsv, t.bc) == (0, P.CROP_NOT_DRAWN, 0, 0, 236, 251, 64, 112, 0, 0)
    with pytest.raises(AssertionError, match="window outside"):
        P.PraPlan(236, 251, 4, P.CROP_RANDOM, 0, 17, 220, 220, 96, 96)          # transposed: the frame is 251 x 236, so x0 <= 16 and y0 <= 31
    assert P.PraPlan(236, 251, 4, P.CROP_RANDOM, 31, 16, 220, 220, 96, 96).frame == (251, 236)


def test_gates_fire_half_the_time_and_every_draw_lies_in_its_support():
    spec = P.PraSpec((96, 96), True)
    n = 4000
    fired = dict.fromkeys(P.GATES + ("center",), 0)
    for i in range(n):
        dr = P.draw_pra(seed=11, epoch=i % 5, index=i)
        for g in fired:
            fired[g] += bool(getattr(dr, g))
        assert dr.k in (0, 1, 2, 3) and dr.d in (-1, 0, 1) and -20 <= dr.hue <= 20 and -30 <= dr.sat <= 30 and -20 <= dr.val <= 20
        assert 0.8 <= dr.alpha <= 1.2 and -0.2 <= dr.beta <= 0.2 and 0 <= dr.u1 < 1 and 0 <= dr.u2 < 1
        for H, W in ((236, 251), (120, 300)):
            p = P.plan_from_draws(spec, H, W, dr)
            th, tw = p.frame
            assert (th, tw) == ((W, H) if dr.transpose != (dr.rot and dr.k % 2 == 1) else (H, W))
            assert p.hsv == dr.hsv and p.bc == dr.bc and 0 <= p.hue_shift <= 255
            if not dr.crop:
                assert p.crop == P.CROP_NOT_DRAWN and (p.y0, p.x0, p.wh, p.ww) == (0, 0, th, tw)
            elif min(th, tw) < 220:                              # skipped exactly when the frame is too small
                assert p.crop == P.CROP_TOO_SMALL and (p.y0, p.x0, p.wh, p.ww) == (0, 0, th, tw)
            elif dr.center:
                assert p.crop == P.CROP_CENTER and (p.y0, p.x0, p.wh, p.ww) == ((th - 220) // 2, (tw - 220) // 2, 220, 220)
            else:
                assert p.crop == P.CROP_RANDOM and (p.y0, p.x0, p.wh, p.ww) == (int((th - 220) * dr.u1), int((tw - 220) * dr.u2), 220, 220)
    for g, c in fired.items():
        assert 0.45 <= c / n <= 0.55, (g, c / n)
    ks = np.bincount([P.draw_pra(1, 0, i).k for i in range(n)], minlength=4) / n
    ds = np.bincount([P.draw_pra(1, 0, i).d + 1 for i in range(n)], minlength=3) / n
    assert np.all(np.abs(ks - 0.25) < 0.05) and np.all(np.abs(ds - 1 / 3) < 0.05)
    assert P.plan_from_draws(P.PraSpec((96, 96), True, crop=100), 120, 300, P.draw_pra(0, 0, 0)._replace(crop=True, center=True)).wh == 100


def test_numpy_restatement_of_sampled_plans_equals_the_pil_oracle():
    pytest.importorskip("PIL")
    spec = P.PraSpec((48, 48), True, crop=60)
    for i in range(24):
        h, w = ((70, 83), (40, 90))[i % 2]
        img, mask = ref.synth_picture(h, w, i), ref.synth_mask(h, w, i)
        p = P.sample_pra_plan(spec, h, w, seed=5, index=i)
        a1, b1 = ref.run_plan_pil(img, mask, p)
        a2, b2 = ref.run_plan_numpy(img, mask, p)
        assert np.array_equal(a1, a2) and np.array_equal(b1, b2), key(p)


# ---- datasets and routing --------------------------------------------------------------------------------------------------------------------------
def write_kvasir(root, folds=(("fold_0", 2, (40, 64)), ("fold_1", 3, (40, 64)), ("fold_2", 1, (32, 48))), binary=False):
    from PIL import Image
    for fold, n, hw in folds:
        for sub in ("images", "masks"):
            os.makedirs(os.path.join(root, "kvasir", fold, sub))
        for i in range(n):
            Image.fromarray(ref.synth_picture(hw[0], hw[1], 100 + i)).save(os.path.join(root, "kvasir", fold, "images", "%s_%05d.png" % (fold[-1], i)))
            m = ref.synth_mask(hw[0], hw[1], 100 + i)
            Image.fromarray((m >= 128).astype(np.uint8) if binary else m).save(os.path.join(root, "kvasir", fold, "masks", "%s_%05d.png" % (fold[-1], i)))


def test_kvasir_fold_dataset_lists_pairs_and_checks_sizes(tmp_path):
    pytest.importorskip("PIL")
    from PIL import Image
    root = str(tmp_path)
    write_kvasir(root)
    cfg = make_cfg(DATASETS__DATASET_DIR=root, DATASETS__SOURCE_TRAIN="polyp_train", DATASETS__TEST="polyp_val", DATASETS__CROSS_VAL=1, AUG__NAME="pra",
                   INPUT__TRAINSIZE=96, INPUT__INPUT_SIZE_TEST=(112, 64))
    src = data.build_dataset(cfg, "train", True)
    assert isinstance(src, datasets.KvasirFoldDataset) and src.device_transform and isinstance(src.transform, P.PraSpec)
    assert [os.path.basename(p) for p in src.image_paths] == ["0_00000.png", "0_00001.png", "2_00000.png"]            # folds 0 and 2, sorted
    assert src.transform.train and (src.transform.out_h, src.transform.out_w, src.transform.crop) == (96, 96, 220)
    image, mask, name = src[2]
    assert image.dtype == torch.uint8 and tuple(image.shape) == (32, 48, 3) and mask.dtype == torch.uint8 and tuple(mask.shape) == (32, 48) and name == "2_00000"
    assert np.array_equal(image.numpy(), ref.synth_picture(32, 48, 100)) and np.array_equal(mask.numpy(), ref.synth_mask(32, 48, 100))
    val = data.build_dataset(cfg, "test", False)
    assert isinstance(val, datasets.KvasirFoldDataset) and [os.path.basename(p) for p in val.image_paths] == ["1_00000.png", "1_00001.png", "1_00002.png"]
    assert not val.transform.train and (val.transform.out_h, val.transform.out_w) == (64, 112)
    assert datasets.has_device_transform(val) and np.array_equal(val.id_table, P.MASK_TABLE)
    # an RGB mask file (as Kvasir-SEG ships them) is read as grey
    Image.fromarray(np.repeat(ref.synth_mask(32, 48, 100)[..., None], 3, 2)).save(src._paths(2)[1])
    assert np.array_equal(src[2][1].numpy(), ref.synth_mask(32, 48, 100))
    # a callable transform is honoured as in the reference
    called = []
    hooked = datasets.KvasirFoldDataset(cfg, os.path.join(root, "kvasir"), mode="train", cross_val=1, transform=lambda a, b: (called.append((a.mode, b.mode)), (1, 2))[1])
    assert hooked[0][:2] == (1, 2) and called == [("RGB", "L")]
    Image.fromarray(ref.synth_mask(30, 48, 1)).save(src._paths(2)[1])
    with pytest.raises(ValueError, match="2_00000.png"):
        src[2]
    from core.datasets.kvasir import KvasirDataSet, KvasirFoldDataset
    assert (KvasirDataSet, KvasirFoldDataset) == (datasets.KvasirDataSet, datasets.KvasirFoldDataset)


def test_routing_of_the_polyp_and_kvasir_names(tmp_path):
    pytest.importorskip("PIL")
    root = str(tmp_path / "data")
    polyp = dict(DATASETS__SOURCE_TRAIN="polyp_train", DATASETS__TEST="polyp_val", DATASETS__CROSS_VAL=0)
    # no directory: synthetic, whatever AUG.NAME says
    for aug in ("pra", "aspp", "attn"):
        cfg = make_cfg(DATASETS__DATASET_DIR=root, AUG__NAME=aug, **polyp)
        assert isinstance(data.build_dataset(cfg, "train", True), data.SyntheticPolyp) and isinstance(data.build_dataset(cfg, "test", False), data.SyntheticPolyp)
        assert data.real_dataset_root(cfg, "polyp_train") is None
    write_kvasir(root, binary=True)
    # the directory exists: polyp_* is read from disk under "pra" only, kvasir_* under "aspp" only
    for aug, want in (("pra", datasets.KvasirFoldDataset), ("aspp", data.SyntheticPolyp), ("attn", data.SyntheticPolyp)):
        cfg = make_cfg(DATASETS__DATASET_DIR=root, AUG__NAME=aug, **polyp)
        assert type(data.build_dataset(cfg, "train", True)) is want and type(data.build_dataset(cfg, "test", False)) is want, aug
    for aug, want in (("aspp", datasets.KvasirDataSet), ("pra", data.SyntheticPolyp), ("attn", data.SyntheticPolyp)):
        cfg = make_cfg(DATASETS__DATASET_DIR=root, AUG__NAME=aug, DATASETS__SOURCE_TRAIN="kvasir_train", DATASETS__TEST="kvasir_val", DATASETS__CROSS_VAL=0,
                       MODEL__NUM_CLASSES=2)
        assert type(data.build_dataset(cfg, "train", True)) is want, aug
    kv = data.build_dataset(make_cfg(DATASETS__DATASET_DIR=root, AUG__NAME="aspp", DATASETS__SOURCE_TRAIN="kvasir_train", DATASETS__CROSS_VAL=0, MODEL__NUM_CLASSES=2), "train", True)
    assert isinstance(kv.transform, augment.AugmentSpec) and kv.device_transform and len(kv) == 4
    assert kv.id_table[0] == 0 and kv.id_table[1] == 1 and np.all(kv.id_table[2:] == 255)
    image, ids, name = kv[0]
    assert ids.dtype == torch.uint8 and set(np.unique(ids.numpy()).tolist()) <= {0, 1} and name == "1_00000"
    # GTA5 under "pra" is still refused
    os.makedirs(os.path.join(root, "gta5"))
    with pytest.raises(ValueError, match="AUG.NAME"):
        data.build_dataset(make_cfg(DATASETS__DATASET_DIR=root, AUG__NAME="pra", DATASETS__SOURCE_TRAIN="gta5_train"), "train", True)
    # the loader dispatches on the spec's type
    cfg = make_cfg(DATASETS__DATASET_DIR=root, AUG__NAME="pra", INPUT__TRAINSIZE=64, **polyp)
    ds = data.build_dataset(cfg, "train", True)
    loader = datasets.wrap_loader(ds, batch_size=2, shuffle=True, num_workers=2, drop_last=True, pin_memory=True, collate_fn=None)
    assert isinstance(loader, datasets.DeviceAugmentLoader) and len(loader) == 2
    plans = loader.plans_for([0, 3], [(40, 64), (32, 48)], epoch=1)
    assert all(isinstance(p, P.PraPlan) for p in plans) and key(plans[1]) == key(P.sample_pra_plan(ds.transform, 32, 48, 0, 1, 3))
    assert key(plans[0]) != key(loader.plans_for([0], [(40, 64)], epoch=2)[0]) or key(plans[0]) != key(loader.plans_for([0], [(40, 64)], epoch=3)[0])


def test_the_kvasir_yaml_loads_and_keeps_the_synthetic_data_without_a_directory(tmp_path):
    cfg = CfgNode(default_tree())
    cfg.merge_from_file(os.path.join(ROOT, "configs", "pranet_src_kvasir.yaml"))
    assert cfg.AUG.NAME == "pra" and cfg.DATASETS.SOURCE_TRAIN == "polyp_train" and cfg.INPUT.TRAINSIZE == 352
    base = CfgNode(default_tree())
    base.merge_from_file(os.path.join(ROOT, "configs", "pranet_src_polyp.yaml"))
    assert base.AUG.NAME != "pra"
    base.merge_from_list(["AUG.NAME", "pra"])
    assert base == cfg                                           # the polyp YAML plus AUG.NAME
    cfg.merge_from_list(["DATASETS.DATASET_DIR", str(tmp_path / "nothing")])
    assert isinstance(data.build_dataset(cfg, "train", True), data.SyntheticPolyp) and isinstance(data.build_dataset(cfg, "test", False), data.SyntheticPolyp)


# ---- C-ABI ---------------------------------------------------------------------------------------------------------------------------------------
def test_pra_entry_is_declared_bound_and_validates_without_a_gpu():
    import __graft_entry__ as entry
    entry.build()
    src = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    m = re.search(r"\bint\s+mi_augment_pra_batch\s*\(([^;{]*)\)\s*;", src)
    assert m and m.group(1).count(",") + 1 == len(_lib.SIGNATURES["mi_augment_pra_batch"][1]) == 8
    assert "augment_pra.hip" in entry.SOURCES
    fields = re.search(r"typedef struct MiPraSample \{(.*?)\} MiPraSample;", src, flags=re.S).group(1)
    declared = [n.strip().split("[")[0] for line in fields.split(";") if line.strip() for n in re.sub(r"^\s*(const\s+)?\w+\*?\s+", "", line.strip()).split(",")]
    assert declared == [f[0] for f in _lib.MiPraSample._fields_]
    assert ctypes.sizeof(_lib.MiPraSample) == 10 * 8 + 14 * 4 + 6 * 4 + 4 * 256              # pointers, ints, floats, tables: no padding
    L = _lib.lib()
    assert L.mi_augment_pra_batch(None, None, 1, 8, 8, None, None, None) == -22 and b"null operand" in L.mi_last_error()
    rec = (_lib.MiPraSample * 1)()
    one = ctypes.c_void_p(64)
    args = (one, ctypes.cast(rec, ctypes.c_void_p), 1, 8, 8, one, None, None)
    assert L.mi_augment_pra_batch(*args) == -22 and b"sample 0: image" in L.mi_last_error()
    r = rec[0]
    r.img, r.H, r.W, r.sym = 64, 16, 24, 8
    assert L.mi_augment_pra_batch(*args) == -22 and b"symmetry 8" in L.mi_last_error()
    r.sym, r.y0, r.x0, r.wh, r.ww = 4, 0, 1, 24, 16                                         # transposed: the frame is 24 x 16
    assert L.mi_augment_pra_batch(*args) == -22 and b"outside the transformed frame" in L.mi_last_error()
    r.x0, r.win, r.wstride = 0, 64, 48
    assert L.mi_augment_pra_batch(*args) == -22 and b"tables exactly when its size changes" in L.mi_last_error()
    r.hcoef = r.hbound = r.vcoef = r.vbound = 64
    r.hk, r.vk = 5, 9                                                                       # 16 -> 8 has 5 taps, 24 -> 8 has 7
    assert L.mi_augment_pra_batch(*args) == -22 and b"taps" in L.mi_last_error()
    r.vk = 7
    assert L.mi_augment_pra_batch(*args) == -22 and b"tmp buffer" in L.mi_last_error()
    r.tmp, r.tstride, r.mask = 64, 24, 64
    assert L.mi_augment_pra_batch(*args) == -22 and b"mask output" in L.mi_last_error()
