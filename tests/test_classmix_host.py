"""CPU tests of the mean-teacher + ClassMix self-training (host/self_train.py AsppClassMix, csrc/classmix.hip): argument validation of the three
entries without a GPU, the selection rule, the config keys and refusals, the EMA schedule, the checkpoint, the entry points, and the literal
(FUSED = False) loop on the oracle's CPU modules."""
import ctypes
import importlib.util
import logging
import os

import numpy as np
import pytest
import torch

import __graft_entry__ as entry
import _classmix_ref as ref
from oracle import ref_model
from rnd_semantic_segmentation_amd import _lib
from rnd_semantic_segmentation_amd.host import config as hc
from rnd_semantic_segmentation_amd.host import plugin, self_train, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "configs", "deeplabv2_r101_classmix.yaml")


def mix_cfg(tmp_path="/tmp", *opts):
    c = hc.CfgNode(hc.default_tree())
    c.merge_from_file(YAML)
    c.merge_from_list(["OUTPUT_DIR", str(tmp_path)] + list(opts))
    return c


@pytest.fixture(scope="module")
def L():
    try:
        return _lib.lib()
    except _lib.MiError as e:
        pytest.fail("libmi355seg.so not built: %s" % e)


ONE = 64          # a non-null, 16-byte aligned dummy address: validation fails before it is dereferenced


def _v(a):
    return None if a is None else ctypes.c_void_p(a)


# ------------------------------------------------------------------------------------------------ argument validation, no GPU
def test_label_classes_refuses_bad_arguments_before_any_launch(L):
    call = lambda labels=ONE, present=ONE, B=1, H=4, W=4, K=19: L.mi_label_classes(_v(labels), _v(present), B, H, W, K, None)
    assert call(labels=None) == -22 and b"null operand" in L.mi_last_error()
    assert call(present=None) == -22 and b"null operand" in L.mi_last_error()
    for K in (0, -1, 33):
        assert call(K=K) == -22 and b"outside 1..32" in L.mi_last_error()
    for kw in (dict(B=0), dict(H=0), dict(W=-3)):
        assert call(**kw) == -22 and b"bad dimension" in L.mi_last_error()


def test_classmix_refuses_bad_arguments_before_any_launch(L):
    names = ("src_img", "tgt_img", "src_lab", "teacher_low", "present", "priority", "mix_img", "mix_lab", "mask", "counts")

    def call(threshold=0.5, ignore=255, B=1, h=2, w=2, K=19, H=8, W=8, **ptr):
        p = {n: ptr.get(n, ONE) for n in names}
        return L.mi_classmix(_v(p["src_img"]), _v(p["tgt_img"]), _v(p["src_lab"]), _v(p["teacher_low"]), _v(p["present"]), _v(p["priority"]),
                             threshold, ignore, _v(p["mix_img"]), _v(p["mix_lab"]), _v(p["mask"]), _v(p["counts"]), B, h, w, K, H, W, None)

    for n in names:
        if n != "mask":                                    # mask may be NULL
            assert call(**{n: None}) == -22 and b"null operand" in L.mi_last_error(), n
    for K in (0, 33):
        assert call(K=K) == -22 and b"outside 1..32" in L.mi_last_error()
    assert call(h=9) == -22 and b"upsampled" in L.mi_last_error()              # H < h
    assert call(w=9) == -22 and b"upsampled" in L.mi_last_error()              # W < w
    for kw in (dict(B=0), dict(h=0), dict(w=0), dict(H=0), dict(W=-1)):
        assert call(**kw) == -22 and b"bad dimension" in L.mi_last_error(), kw
    for t in (-0.01, 1.01, float("nan")):
        assert call(threshold=t) == -22 and b"threshold" in L.mi_last_error()
    assert call(ignore=3) == -22 and b"ignore_index" in L.mi_last_error()


def test_ema_update_refuses_bad_arguments_before_any_launch(L):
    call = lambda t=ONE, s=ONE, n=8, hyper=ONE: L.mi_ema_update(_v(t), _v(s), n, _v(hyper), None)
    for kw in (dict(t=None), dict(s=None), dict(hyper=None)):
        assert call(**kw) == -22 and b"null operand" in L.mi_last_error()
    assert call(n=0) == -22 and b"n = 0" in L.mi_last_error()
    assert call(t=ONE + 2) == -22 and b"4-byte aligned" in L.mi_last_error()
    assert call(s=ONE + 1) == -22 and b"4-byte aligned" in L.mi_last_error()


def test_wrappers_have_no_cpu_path():
    from rnd_semantic_segmentation_amd import kernels
    with pytest.raises(_lib.MiError, match="GPU"):
        kernels.label_classes(torch.zeros(1, 4, 4, dtype=torch.int64), 19)
    with pytest.raises(_lib.MiError, match="GPU"):
        kernels.ema_update(torch.zeros(4), torch.zeros(4), torch.zeros(1))


# ------------------------------------------------------------------------------------------------ the selection rule
def _bits(classes):
    return sum(1 << c for c in classes)


def test_selection_rule_on_hand_made_cases():
    K = 19
    prio = np.arange(K)[::-1].copy()                       # class 18 has the smallest priority
    assert ref.chosen_classes(0, prio, K) == 0                                             # n = 0: the empty set
    assert ref.chosen_classes(_bits([7]), prio, K) == _bits([7])                           # n = 1: ceil(1/2) = 1
    assert ref.chosen_classes(_bits([2, 11]), prio, K) == _bits([11])                      # n = 2: the one of smaller priority
    assert ref.chosen_classes(_bits([0, 3, 5, 8, 13]), prio, K) == _bits([13, 8, 5])       # n = 5: ceil(5/2) = 3
    prio2 = np.arange(K)
    assert ref.chosen_classes(_bits([0, 3, 5, 8, 13]), prio2, K) == _bits([0, 3, 5])
    # K = 32: class 31 is bit 31
    p32 = np.arange(32)[::-1].copy()
    assert ref.chosen_classes(_bits([31, 4]), p32, 32) == _bits([31])
    assert ref.chosen_classes(_bits([31]), np.arange(32), 32) == 1 << 31


def test_present_bits_ignore_and_out_of_range_labels():
    lab = np.full((3, 4, 5), 255, dtype=np.int64)
    lab[1, 0, 0], lab[1, 3, 4], lab[1, 2, 2], lab[1, 1, 1] = 31, 0, -1, 32
    lab[2, :, :] = 19                                      # out of range for K = 19, in range for K = 32
    assert ref.present_bits(lab, 32).tolist() == [0, (1 << 31) | 1, 1 << 19]
    assert ref.present_bits(lab, 19).tolist() == [0, 1, 0]
    assert ref.present_bits(lab, 19).dtype == np.uint32


def test_classmix_restatement_counts_and_mask():
    K = 4
    src_lab = np.array([[[0, 0, 1, 255], [2, 2, 1, 7]]], dtype=np.int64)
    pseudo = np.array([[[3, 255, 3, 1], [255, 0, 2, 2]]], dtype=np.uint8)
    src, tgt = np.ones((1, 3, 2, 4), np.float32), np.zeros((1, 3, 2, 4), np.float32)
    present = ref.present_bits(src_lab, K)
    assert present.tolist() == [0b0111]
    prio = np.array([[3, 0, 1, 2]], dtype=np.uint8)        # classes 1 and 2 are chosen (ceil(3/2) = 2)
    img, lab, mask, counts = ref.classmix(src, tgt, src_lab, pseudo, present, prio, K, 255)
    assert mask.tolist() == [[[0, 0, 1, 0], [1, 1, 1, 0]]]
    assert lab.tolist() == [[[3, 255, 1, 1], [2, 2, 1, 2]]]
    assert (img[0, 1] == mask[0]).all() and counts.tolist() == [[4, 3]]


# ------------------------------------------------------------------------------------------------ config keys, refusals, schedule
def test_config_keys_and_ranges(tmp_path):
    c = hc.CfgNode(hc.default_tree())
    assert c.SOLVER.EMA_ALPHA == 0.99 and c.SOLVER.MIX_THRESHOLD == 0.968
    assert hc._RANGES["SOLVER.EMA_ALPHA"] == (0.0, 1.0) and hc._RANGES["SOLVER.MIX_THRESHOLD"] == (0.0, 1.0)
    for key in ("SOLVER.EMA_ALPHA", "SOLVER.MIX_THRESHOLD"):
        for bad in (-0.1, 1.5):
            with pytest.raises(ValueError, match=key):
                mix_cfg(tmp_path, key, bad)
    m = mix_cfg(tmp_path)
    assert m.MODEL.FREEZE_BN is True and m.MODEL.NUM_CLASSES == 19 and m.SOLVER.LOSS == "ce"
    assert tuple(m.INPUT.SOURCE_INPUT_SIZE_TRAIN) == tuple(m.INPUT.TARGET_INPUT_SIZE_TRAIN) == (1024, 512)
    assert m.DATASETS.SOURCE_TRAIN == "gta5_train" and m.DATASETS.TARGET_TRAIN == "cityscapes_train"


def test_keys_are_refused_outside_the_combo(tmp_path):
    assert plugin.self_train_options(mix_cfg(tmp_path), "ASPPTrainer") is None                    # at the defaults every trainer is as it was
    assert plugin.self_train_options(mix_cfg(tmp_path), "AsppClassMix", True) == (0.99, 0.968)
    for key, v in (("SOLVER.EMA_ALPHA", 0.999), ("SOLVER.MIX_THRESHOLD", 0.9)):
        with pytest.raises(NotImplementedError, match="aspp_classmix"):
            plugin.self_train_options(mix_cfg(tmp_path, key, v), "ASPPTrainer")
    assert plugin.self_train_options(mix_cfg(tmp_path, "SOLVER.EMA_ALPHA", 0.999, "SOLVER.MIX_THRESHOLD", 0.9), "x", True) == (0.999, 0.9)
    assert plugin.BaseTrainer.SELF_TRAINING is False and self_train.ClassMixStudent.SELF_TRAINING is True
    from rnd_semantic_segmentation_amd.host import trainer as tr
    assert issubclass(self_train.ClassMixStudent, tr.ASPPTrainer) and self_train.AsppClassMix.trainer_cls is self_train.ClassMixStudent


def test_ema_schedule():
    assert [self_train.ema_alpha(i, 0.99) for i in range(3)] == [0.0, 0.5, 1.0 - 1.0 / 3.0]
    assert self_train.ema_alpha(98, 0.99) == 1.0 - 1.0 / 99 and self_train.ema_alpha(99, 0.99) == 0.99 and self_train.ema_alpha(10 ** 6, 0.99) == 0.99
    assert self_train.ema_alpha(5, 0.5) == 0.5 and self_train.ema_alpha(0, 0.0) == 0.0


def test_priorities_are_permutations_seeded_by_iteration_and_rank():
    p = self_train.draw_priorities(3, 0, 4, 19)
    assert p.dtype == torch.uint8 and tuple(p.shape) == (4, 19)
    assert all(sorted(row.tolist()) == list(range(19)) for row in p)
    assert torch.equal(p, self_train.draw_priorities(3, 0, 4, 19))
    assert not torch.equal(p, self_train.draw_priorities(4, 0, 4, 19)) and not torch.equal(p, self_train.draw_priorities(3, 1, 4, 19))


# ------------------------------------------------------------------------------------------------ the combo on the oracle's CPU modules
def _batches(n, seed0, size=33):
    out = []
    for i in range(n):
        x = torch.from_numpy(synth.synth_image(2, size, size, seed=seed0 + i))
        y = torch.from_numpy(synth.synth_label(2, size, size, 19, seed=seed0 + i))
        out.append((x, y, ["n%d" % i] * 2))
    return out


def _cpu_combo(tmp_path, monkeypatch, *opts, resume=""):
    from rnd_semantic_segmentation_amd.host import trainer as tr
    cfg = mix_cfg(tmp_path, "SOLVER.EPOCHS", 2, "SOLVER.BASE_LR", 5e-4, "SOLVER.MIX_THRESHOLD", 0.0634, "resume", resume, *opts)
    cfg.freeze()

    def formula(m):
        synth.load_formula_weights(m)
        return m

    monkeypatch.setattr(tr.ASPPTrainer, "build_feature_extractor", staticmethod(lambda cfg: formula(ref_model.RefFeatureExtractor((1, 1, 1, 1)))))
    monkeypatch.setattr(tr.ASPPTrainer, "build_classifier", staticmethod(lambda cfg: formula(ref_model.RefASPP())))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(self_train, "setup_logger", lambda *a, **k: logging.getLogger("test_classmix_%s" % tmp_path.name))
    return self_train.AsppClassMix("aspp_classmix", cfg, _batches(3, 60), _batches(3, 80), 0)


def test_refusals(tmp_path, monkeypatch):
    with pytest.raises(NotImplementedError, match="FREEZE_BN"):
        _cpu_combo(tmp_path, monkeypatch, "MODEL.FREEZE_BN", False)
    with pytest.raises(NotImplementedError, match="SOLVER.LOSS"):
        _cpu_combo(tmp_path, monkeypatch, "SOLVER.LOSS", "ohem")
    with pytest.raises(NotImplementedError, match="SOLVER.LOSS"):
        _cpu_combo(tmp_path, monkeypatch, "SOLVER.LOSS", "gdl")
    combo = _cpu_combo(tmp_path, monkeypatch)
    from rnd_semantic_segmentation_amd.host import fada, trainer as tr
    with pytest.raises(NotImplementedError, match="aspp_classmix"):          # a plain trainer (builders patched above) refuses the changed key
        tr.ASPPTrainer("aspp", combo.cfg, [], 0, logging.getLogger("test_classmix_plain"))
    monkeypatch.setattr(fada, "setup_logger", lambda *a, **k: logging.getLogger("test_classmix_fada"))
    with pytest.raises(NotImplementedError, match="aspp_classmix"):          # ... and so does another combo
        fada.AsppFada("aspp_fada", combo.cfg, [], [], 0)
    xs, ys, _ = _batches(1, 60)[0]
    with pytest.raises(ValueError, match="one shape"):
        combo.train_step(xs, ys, torch.zeros(2, 3, 33, 41), 10)
    with pytest.raises(ValueError, match="one shape"):
        combo.train_step(xs, ys, torch.zeros(1, 3, 33, 33), 10)
    assert combo.iteration == 0
    with pytest.raises(_lib.MiError, match="GPU"):         # FUSED on the CPU: no quiet fall-back to torch ops
        combo.train_step(xs, ys, xs.clone(), 10)


def test_literal_mixing_matches_the_restatement(tmp_path, monkeypatch):
    combo = _cpu_combo(tmp_path, monkeypatch)
    combo.FUSED, combo.KEEP_MIX = False, True
    (xs, ys, _), (xt, _, _) = _batches(1, 60)[0], _batches(1, 80)[0]
    ys = ys.clone()
    ys[0, :5] = 255
    ys[1] = 4                                              # a one-class image: everything is pasted
    low = combo._teacher_low(xt)
    r = combo.train_step(xs, ys, xt, 10)
    img, lab = (t.numpy() for t in combo.last_mix)
    prob = torch.softmax(torch.nn.functional.interpolate(low.permute(0, 3, 1, 2), size=(33, 33), mode="bilinear", align_corners=True), 1)
    conf, arg = prob.max(1)
    pseudo = torch.where(conf >= combo.threshold, arg, torch.full_like(arg, 255)).to(torch.uint8).numpy()
    assert 0 < int((pseudo == 255).sum()) < pseudo.size     # the threshold splits the picture
    labs = ys.long().numpy()
    prio = self_train.draw_priorities(0, 0, 2, 19).numpy()
    want = ref.classmix(xs.numpy(), xt.numpy(), labs, pseudo, ref.present_bits(labs, 19), prio, 19, 255)
    assert np.array_equal(img, want[0]) and np.array_equal(lab, want[1]) and np.array_equal(r["counts"].numpy(), want[3])
    assert want[3][1].tolist() == [33 * 33, 0] and 0 < want[3][0][0] < 28 * 33
    assert np.isfinite(float(r["loss"])) and combo.iteration == 1


def test_literal_loop_checkpoint_and_resume(tmp_path, monkeypatch):
    combo = _cpu_combo(tmp_path, monkeypatch)
    combo.FUSED = False
    state = lambda m: {k: v.detach().clone() for k, v in m.state_dict().items()}
    combo.train()
    assert combo.iteration == 6 and len(combo.loss_data) == 6 and all(np.isfinite(combo.loss_data))
    assert len(combo.kept_data) == 6 and all(0.0 <= v <= 1.0 for v in combo.kept_data + combo.pasted_data)
    s, t = state(combo.aspp.classifier), state(combo.teacher_classifier)
    assert any(not torch.equal(s[k], t[k]) for k in s)     # after six updates the teacher lags the student
    assert os.path.exists(tmp_path / "aspp_classmix_chart_params.json")
    path = tmp_path / "AsppClassMix-2.pth"
    ck = torch.load(path, map_location="cpu")
    assert set(ck) == {"mix_epoch", "iteration", "feature_extractor", "classifier", "optimizer_fea", "optimizer_cls", "teacher_feature_extractor",
                       "teacher_classifier"}
    assert ck["iteration"] == 6 and ck["mix_epoch"] == 2
    assert list(ck["feature_extractor"]) == list(ck["teacher_feature_extractor"]) and list(ck["classifier"]) == list(ck["teacher_classifier"])
    # what ASPPTester._load_checkpoint reads is the student
    fe, cls = ref_model.RefFeatureExtractor((1, 1, 1, 1)), ref_model.RefASPP()
    fe.load_state_dict(ck["feature_extractor"])
    cls.load_state_dict(ck["classifier"])
    assert all(torch.equal(v, s[k]) for k, v in cls.state_dict().items())
    # resume: both nets restored, the position too
    again = _cpu_combo(tmp_path, monkeypatch, resume=str(path))
    assert again.iteration == 6 and again.start_epoch == 3
    assert all(torch.equal(v, t[k]) for k, v in again.teacher_classifier.state_dict().items())
    assert all(torch.equal(v, s[k]) for k, v in again.aspp.classifier.state_dict().items())
    # a source-only checkpoint: the teacher is the student's copy, the schedule starts at 0
    src_only = {k: ck[k] for k in ("feature_extractor", "classifier")}
    src_only["epoch"] = 3
    torch.save(src_only, tmp_path / "Aspp-3.pth")
    fresh = _cpu_combo(tmp_path, monkeypatch, resume=str(tmp_path / "Aspp-3.pth"))
    assert fresh.iteration == 0 and fresh.start_epoch == 1
    assert all(torch.equal(v, s[k]) for k, v in fresh.teacher_classifier.state_dict().items())


# ------------------------------------------------------------------------------------------------ entry points and documents
def test_train_adv_dispatch_reaches_the_combo(tmp_path, monkeypatch):
    spec = importlib.util.spec_from_file_location("train_adv_classmix_mod", os.path.join(ROOT, "train_adv.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    seen = {}

    class Recorder:
        def __init__(self, name, cfg, src_loader, tgt_loader, local_rank):
            seen.update(name=name, src=src_loader, tgt=tgt_loader, rank=local_rank)

    monkeypatch.setattr(self_train, "AsppClassMix", Recorder)
    monkeypatch.setattr(mod, "run_trainer", lambda trainer, *loaders: seen.update(trainer=trainer, loaders=loaders))
    cfg = mix_cfg(tmp_path, "DATASETS.DATASET_DIR", str(tmp_path / "none"))
    mod.main("aspp_classmix", cfg, 0)
    assert seen["name"] == "aspp_classmix" and isinstance(seen["trainer"], Recorder) and seen["loaders"] == (seen["src"], seen["tgt"])
    assert seen["src"].batch_size == seen["tgt"].batch_size == 4
    with pytest.raises(NotImplementedError, match="aspp_classmix"):
        mod.main("attn_fada", cfg, 0)


def test_dropin_and_documents():
    from core.combos.aspp_classmix import AsppClassMix
    assert AsppClassMix is self_train.AsppClassMix and AsppClassMix.FUSED is True
    assert "classmix.hip" in entry.SOURCES
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "deeplabv2_r101_classmix.yaml" in readme and "aspp_classmix" in readme
    assert "mi_classmix" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "aspp_classmix" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
