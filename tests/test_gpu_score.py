"""GPU side of the fused evaluation tail: mi_upsample_predict_score (csrc/upsample_infer.hip) against the probability kernel it shares its arithmetic
with (zero differences allowed), its counts against host/metrics.py on the same mask, the reference's own masks and metrics (g14 / g6 fixtures, the
rule of tests/_multiscale.py), ASPPTester with TEST.FUSED_SCORE True against False (same matrix, lines, JSON and PNG bytes) and the two scripts
of the self-distillation stage on a tiny Cityscapes tree."""
import json
import logging
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _augment_ref as ref
import _cases
import _multiscale as ms
from rnd_semantic_segmentation_amd.host import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = None
M = None


@pytest.fixture(scope="module", autouse=True)
def _kern():
    global K, M
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from rnd_semantic_segmentation_amd import kernels
    from rnd_semantic_segmentation_amd.host import metrics
    K, M = kernels, metrics
    yield


def _cfg(Kc):
    from rnd_semantic_segmentation_amd.host import config as hc
    cfg = hc.cfg.clone()
    cfg.defrost()
    cfg.merge_from_list(["MODEL.NUM_CLASSES", Kc])
    return cfg


def _lows(Kc, sizes, tag):
    return [torch.from_numpy((synth.uniform("score.%s.%d" % (tag, i), (h, w, Kc)) * 6).astype(np.float32)).cuda() for i, (h, w) in enumerate(sizes)]


def _labels(Kc, hw, seed):
    """Every class, plus -1, K, 254, 255 and 300 on about a third of the pixels."""
    g = np.random.RandomState(seed)
    lab = g.randint(0, Kc, size=hw).astype(np.int64)
    odd = np.array([-1, Kc, 254, 255, 300], dtype=np.int64)
    where = g.rand(*hw) < 0.3
    lab[where] = odd[g.randint(0, odd.size, size=int(where.sum()))]
    return torch.from_numpy(lab).cuda()


def _want_counts(Kc, pred, lab, ignore_index):
    """[K*K + 3K] from host/metrics.py on a mask: cmt, intersection, output, target."""
    cmt = M.confusion_matrix(_cfg(Kc), pred.flatten(), lab.flatten())
    ai, _, at, ao = M.intersectionAndUnionGPU(pred.long().clone(), lab.clone(), Kc, ignore_index)
    return torch.cat([cmt.flatten(), ai.long().cpu(), ao.long().cpu(), at.long().cpu()])


SIX = [(9, 13), (17, 22), (12, 19), (25, 31), (5, 7), (21, 40)]       # tests/test_gpu_multiscale.py: six source sizes
SIX_MIRRORS = [False, True, False, True, False, True]
SIZES = [(77, 150), (77, 151), (33, 64), (15, 30)]


def _sources(Kc, n):
    if n == 1:
        return _lows(Kc, [(9, 13)], "one%d" % Kc), [False], 1.0, 1.0
    return _lows(Kc, SIX, "six%d" % Kc), SIX_MIRRORS, 3.0, 2.0


# ------------------------------------------------------------------------------------------------ kernel against kernel
@pytest.mark.parametrize("n", [1, 6])
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("Kc", [2, 19, 32])
def test_masks_equal_the_probability_kernels_argmax_on_every_pixel(Kc, size, n):
    lows, mirrors, da, db = _sources(Kc, n)
    probs = K.upsample_softmax_multi(lows, mirrors, size, da, db)
    top = probs.max(1)
    want = top[1][0].to(torch.uint8)
    pred, pseudo, counts = K.upsample_predict_score(lows, mirrors, size, da, db)
    assert pseudo is None and counts is None and pred.dtype == torch.uint8 and pred.shape == size
    nd = int((pred != want).sum())
    print("predict_score n=%d K=%d %s: %d of %d pixels differ from max(1) of the probability kernel" % (n, Kc, size, nd, want.numel()))
    assert nd == 0
    assert np.array_equal(pred.cpu().numpy(), probs[0].cpu().numpy().argmax(0))
    for t in (0.0, 0.5, 0.9, 1.0):
        p2, pseudo, _ = K.upsample_predict_score(lows, mirrors, size, da, db, threshold=t, want_pseudo=True)
        wantp = torch.where(top[0][0] >= t, want, torch.full_like(want, 255))
        assert torch.equal(p2, want) and torch.equal(pseudo, wantp), (t, int((pseudo != wantp).sum()))
        if t == 0.0:
            assert torch.equal(pseudo, pred)
    if n == 1:                                                # the single-scale tail (tests/test_gpu_multiscale.py:63 pins the probabilities)
        single, _ = K.upsample_softmax(lows[0][None], size, want_pred=False)
        assert torch.equal(pred, single.max(1)[1][0].to(torch.uint8))


def _tie_maps(Kc):
    """Logit maps whose probabilities tie bit for bit: constant maps, equal channels, and a pair of logits one ulp apart that exp merges (the
    LARGER logit sits at the higher index: the argmax of the logits is not the answer)."""
    h, w = 7, 9
    lo, hi, third = (Kc // 2 if Kc > 2 else 0), Kc - 1, (1 if Kc > 2 else 0)
    base = (synth.uniform("score.tie.%d" % Kc, (h, w, Kc)) * 4).astype(np.float32) - 6.0          # every other class well below
    const = np.zeros((h, w, Kc), np.float32)
    two = base.copy()
    two[..., hi] = two[..., lo] = 3.0
    three = base.copy()
    three[..., hi] = three[..., lo] = three[..., third] = 3.0
    ulp = base.copy()
    ulp[..., lo] = np.float32(0.3)
    ulp[..., hi] = np.nextafter(np.float32(0.3), np.float32(1.0))       # exp(-3e-8) rounds to 1: both classes get the probability of the maximum
    return {"const": const, "two": two, "three": three, "ulp": ulp}, (lo, hi, third)


@pytest.mark.parametrize("size", [(31, 40), (31, 41)])
@pytest.mark.parametrize("Kc", [2, 19, 32])
def test_ties_choose_the_lowest_index_like_torch_max_and_numpy_argmax(Kc, size):
    maps, (lo, hi, third) = _tie_maps(Kc)
    for tag, m in maps.items():
        low = torch.from_numpy(m).cuda()
        for lows, mirrors, da, db in (([low], [False], 1.0, 1.0), ([low, low, low], [False, True, False], 3.0, 1.0)):
            probs = K.upsample_softmax_multi(lows, mirrors, size, da, db)
            pred, _, _ = K.upsample_predict_score(lows, mirrors, size, da, db)
            pn = probs[0].cpu().numpy()
            srt = np.sort(pn, 0)
            ties = int((srt[-1] == srt[-2]).sum())
            print("ties %s K=%d %s n=%d: %d of %d pixels have bit-equal top-2 probabilities" % (tag, Kc, size, len(lows), ties, pred.numel()))
            assert torch.equal(pred, probs.max(1)[1][0].to(torch.uint8))
            assert np.array_equal(pred.cpu().numpy(), pn.argmax(0))
            if tag != "ulp" and len(lows) == 1:
                assert ties == pred.numel()                       # the probabilities DO tie: the rule is exercised on every pixel
                first = {"const": 0, "two": lo, "three": min(lo, third)}[tag]
                assert int(pred.min()) == first and int(pred.max()) == first
            if tag == "ulp" and len(lows) == 1:
                # at the corner pixel the interpolation returns the logits themselves: they differ, their probabilities do not, the lower index wins
                assert m[0, 0, hi] > m[0, 0, lo] and pn[hi, 0, 0] == pn[lo, 0, 0] and int(pred[0, 0]) == lo
                assert ties > 0


# ------------------------------------------------------------------------------------------------ counts
@pytest.mark.parametrize("ignore_index", [255, 250])
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("Kc", [2, 19, 32])
def test_counts_equal_host_metrics_on_the_mask(Kc, size, ignore_index):
    lows, mirrors, da, db = _sources(Kc, 6)
    lab = _labels(Kc, size, 7 + Kc)
    pred, pseudo, counts = K.upsample_predict_score(lows, mirrors, size, da, db, labels=lab, ignore_index=ignore_index, threshold=0.9, want_pseudo=True)
    want = _want_counts(Kc, pred, lab, ignore_index)
    assert counts.dtype == torch.int64 and counts.shape == (Kc * Kc + 3 * Kc,)
    assert torch.equal(counts.cpu(), want), (counts.cpu() - want).nonzero().flatten().tolist()[:8]
    cmt, ai, ao, at = K.split_counts(counts.cpu(), Kc)
    assert int(cmt.sum()) == int(at.sum()) > 0 and int(ao.sum()) > int(at.sum()) and torch.equal(ai, cmt.diagonal())
    # the counts never depend on the threshold; two runs are bit-equal; labels=None writes only the masks
    p0, _, c0 = K.upsample_predict_score(lows, mirrors, size, da, db, labels=lab, ignore_index=ignore_index)
    assert torch.equal(p0, pred) and torch.equal(c0, counts)
    p1, ps1, c1 = K.upsample_predict_score(lows, mirrors, size, da, db, threshold=0.9, want_pseudo=True)
    assert c1 is None and torch.equal(p1, pred) and torch.equal(ps1, pseudo)


def test_two_launches_into_one_buffer_add_up():
    from rnd_semantic_segmentation_amd import _lib
    import ctypes
    Kc, size = 19, (77, 150)
    lows, mirrors, da, db = _sources(Kc, 6)
    lab_a, lab_b = _labels(Kc, size, 1), _labels(Kc, size, 2)
    _, _, ca = K.upsample_predict_score(lows, mirrors, size, da, db, labels=lab_a)
    _, _, cb = K.upsample_predict_score(lows[:1], mirrors[:1], size, 1.0, 1.0, labels=lab_b)
    both = torch.zeros_like(ca)
    pred = torch.empty(size, dtype=torch.uint8, device="cuda")
    for ls, mm, d, e, lab in ((lows, mirrors, da, db, lab_a), (lows[:1], mirrors[:1], 1.0, 1.0, lab_b)):
        src = (_lib.MiProbSource * len(ls))()
        for i, (low, m) in enumerate(zip(ls, mm)):
            src[i].low, src[i].h, src[i].w, src[i].mirror = low.data_ptr(), low.shape[0], low.shape[1], int(m)
        rc = _lib.lib().mi_upsample_predict_score(ctypes.cast(src, ctypes.c_void_p), len(ls), Kc, size[0], size[1], d, e, lab.data_ptr(), 255, 0.0,
                                                  pred.data_ptr(), None, both.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0
    assert torch.equal(both, ca + cb) and int(cb.sum()) > 0


def test_refusals_through_the_wrapper():
    from rnd_semantic_segmentation_amd._lib import MiError
    lows = _lows(19, [(5, 7)] * 17, "bad")
    lab = _labels(19, (33, 33), 3)
    with pytest.raises(MiError):
        K.upsample_predict_score(lows, [False] * 17, (33, 33), 3.0)
    with pytest.raises(MiError):
        K.upsample_predict_score([], [], (33, 33), 3.0)
    with pytest.raises(MiError, match="zero divisor"):
        K.upsample_predict_score(lows[:2], [False, True], (33, 33), 0.0)
    with pytest.raises(MiError, match="ignore_index"):
        K.upsample_predict_score(lows[:2], [False, True], (33, 33), 2.0, labels=lab, ignore_index=3)
    with pytest.raises(MiError, match="threshold"):
        K.upsample_predict_score(lows[:2], [False, True], (33, 33), 2.0, threshold=1.5)
    with pytest.raises(MiError, match="labels must be"):
        K.upsample_predict_score(lows[:2], [False, True], (33, 34), 2.0, labels=lab)


def test_memory_less_than_one_class_plane_at_1024x2048():
    Kc, H, W = 19, 1024, 2048
    lows, mirrors, da, db = _sources(Kc, 6)
    lab = _labels(Kc, (H, W), 5)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    pred, pseudo, counts = K.upsample_predict_score(lows, mirrors, (H, W), da, db, labels=lab, threshold=0.9, want_pseudo=True)
    torch.cuda.synchronize()
    fused = torch.cuda.max_memory_allocated() - base
    want = _want_counts(Kc, pred, lab, 255)
    assert torch.equal(counts.cpu(), want) and int(counts[:Kc * Kc].sum()) == int(((lab >= 0) & (lab < Kc)).sum())
    del pred, pseudo, counts, want
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    probs = K.upsample_softmax_multi(lows, mirrors, (H, W), da, db)
    torch.cuda.synchronize()
    literal = torch.cuda.max_memory_allocated() - base
    print("1024x2048, K=19: predict_score allocates %d bytes (one class plane: %d), the probability tail %d" % (fused, 4 * H * W, literal))
    assert fused < 4 * H * W
    assert literal >= Kc * 4 * H * W
    del probs


# ------------------------------------------------------------------------------------------------ against the reference
@pytest.fixture(scope="module")
def r101():
    from rnd_semantic_segmentation_amd.host import modules
    fe = modules.resnet_feature_extractor("resnet101", freeze_bn=True, pretrained_backbone=False)
    cls = modules.ASPP_Classifier_V2(2048, [6, 12, 18, 24], [6, 12, 18, 24], 19)
    synth.load_formula_weights(fe)
    synth.load_formula_weights(cls)
    return fe.cuda().eval().set_precision("fp32"), cls.cuda().eval().set_precision("fp32")


def _own_counts_parity(r, g, flips, what):
    """The kernel's own counts against the fixture's cmt / iu (the reference's functions' outputs) and summary lines."""
    cmt = r.cmt.numpy()
    iu = [t.numpy() for t in (r.intersection, r.union, r.target, r.output)]
    d_cmt = int(np.abs(cmt - g["cmt"]).sum())
    d_iu = float(np.abs(np.stack(iu) - g["iu"]).sum())
    print("%s: fused counts vs the reference's: |d cmt| %d, |d iu| %.0f, %d flips" % (what, d_cmt, d_iu, flips))
    assert d_cmt <= 2 * flips and d_iu <= 4 * flips, (d_cmt, d_iu, flips)
    if flips == 0:
        assert np.array_equal(cmt, g["cmt"]) and np.array_equal(np.stack(iu), g["iu"])
        meter = M.AverageMeter()
        meter.update(*[a.astype(np.float64) for a in iu])
        lines = []
        meter.summary(type("L", (), {"info": lambda self, s: lines.append(s)})(), 19)
        assert lines == list(g["summary"]), (lines[:2], list(g["summary"][:2]))


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("name", sorted(ms.R101_CASES))
def test_r101_multi_scale_fused_masks_and_counts_equal_reference(r101, name, flip):
    fe, cls = r101
    hw, seed = ms.R101_CASES[name]
    g = ms.load("g14_r101_%s_%s" % (name, ms.flip_tag(flip)))
    x, lab = ms.inputs(hw, seed)
    r = M.predict_and_score(fe, cls, torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda().long(), flip=flip, scales=(0.7, 1.0, 1.3),
                            num_classes=19, ignore_index=255)
    assert r.pred.dtype == torch.uint8 and r.pred.shape == hw and r.pseudo is None
    what = "fused r101@%s multi-scale %s" % (name, ms.flip_tag(flip))
    flips = ms.mask_parity(r.pred.cpu().numpy(), g, what)
    ms.eval_parity(r.pred[None].long(), lab, g, flips, what)
    _own_counts_parity(r, g, flips, what)


@pytest.mark.parametrize("name,size,seed", [("g6_r101_129", 129, 21), ("g6_r101_512x1024", (512, 1024), 31)])
def test_r101_single_scale_fused_masks_and_counts_equal_reference(r101, name, size, seed):
    """The rule of tests/test_gpu_fp32.py:47-70 on the single-scale fixtures."""
    import test_gpu_fp32 as f32
    fe, cls = r101
    g = _cases.load(name)
    gp = _cases.load(name + "_pred")["pred"] if name.endswith("1024") else g["pred"]
    x, lab = _cases.net_inputs(1, size, seed)
    r = M.predict_and_score(fe, cls, torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda().long(), num_classes=19)
    what = "fused " + name
    flips = f32.mask_parity(r.pred.cpu().numpy(), g, gp, what)
    assert f32.FLIP_MARGIN == ms.FLIP_MARGIN
    f32.eval_parity(r.pred[None].long(), lab, g, flips, what)
    _own_counts_parity(r, g, flips, what)


# ------------------------------------------------------------------------------------------------ tester end to end
class _Lines:
    def __init__(self):
        self.lines = []

    def info(self, s):
        self.lines.append(s)

    warning = info


def _run_tester(out, saveres, *opts):
    from core.configs import cfg as global_cfg
    from core.datasets.build import build_dataset
    from core.testers.aspp_tester import ASPPTester
    cfg = global_cfg.clone()
    cfg.defrost()
    cfg.merge_from_list(["MODEL.FREEZE_BN", True, "MODEL.NUM_CLASSES", 19, "OUTPUT_DIR", str(out), "INPUT.INPUT_SIZE_TEST", (161, 97),
                         "PSEUDO_DIR", str(out / "pseudo"), "DATASETS.TEST", "cityscapes_val"] + list(opts))
    os.environ["MI_SYNTH_LEN"] = "2"
    try:
        data = build_dataset(cfg, mode="test", is_source=False)
        loader = torch.utils.data.DataLoader(data, batch_size=1, shuffle=False)
        log = _Lines()
        palette = [(5 * i) % 256 for i in range(768)]
        tester = ASPPTester(cfg, torch.device("cuda"), loader, log, palette, {i: str(i) for i in range(19)}, saveres=saveres)
    finally:
        os.environ.pop("MI_SYNTH_LEN", None)
    synth.load_formula_weights(tester.feature_extractor)
    synth.load_formula_weights(tester.classifier)
    cmt = tester.test()
    js = (out / "aspp_confusion_matrix.json").read_bytes()
    folder = out / "pseudo" / "inference" / "cityscapes_val"
    pngs = {f: (folder / f).read_bytes() for f in sorted(os.listdir(folder))} if saveres else {}
    return cmt, js, log.lines, pngs


@pytest.mark.parametrize("tag,saveres,opts", [
    ("default", False, ()),
    ("ms_flip", False, ("TEST.SCALES", "(0.7, 1.0, 1.3)", "TEST.FLIP", "True")),
    ("bf16", False, ("TEST.PRECISION", "bf16")),
    ("saveres_t0", True, ()),
    ("saveres_t09", True, ("TEST.PSEUDO_THRESHOLD", "0.9")),
    ("saveres_t09_ms_flip", True, ("TEST.PSEUDO_THRESHOLD", "0.9", "TEST.SCALES", "(0.7, 1.0, 1.3)", "TEST.FLIP", "True")),
])
def test_aspp_tester_fused_equals_literal(tmp_path, monkeypatch, tag, saveres, opts):
    from rnd_semantic_segmentation_amd.host import tester as te
    called = []
    real = te.predict_and_score
    monkeypatch.setattr(te, "predict_and_score", lambda *a, **k: (called.append(1), real(*a, **k))[1])
    (tmp_path / "fused").mkdir()
    (tmp_path / "literal").mkdir()
    f = _run_tester(tmp_path / "fused", saveres, "TEST.FUSED_SCORE", "True", *opts)
    assert len(called) == 2                                     # the fused default took the new path ...
    lit = _run_tester(tmp_path / "literal", saveres, "TEST.FUSED_SCORE", "False", *opts)
    assert len(called) == 2                                     # ... and False did not
    assert torch.equal(f[0], lit[0]) and int(f[0].sum()) > 0
    assert f[1] == lit[1]
    assert f[2] == lit[2] and len(f[2]) == 2 + 2 * 19
    assert f[3] == lit[3] and len(f[3]) == (2 if saveres else 0)
    if saveres:
        from PIL import Image
        import io
        masks = [np.array(Image.open(io.BytesIO(b))) for b in f[3].values()]
        n255 = sum(int((m == 255).sum()) for m in masks)
        print("tester %s: %d of %d saved pixels are 255" % (tag, n255, sum(m.size for m in masks)))
        if "t09" not in tag:
            assert n255 == 0 and all(m.max() < 19 for m in masks)


# ------------------------------------------------------------------------------------------------ the scripts of the stage
def _run(args):
    return subprocess.run([sys.executable] + args, cwd=ROOT, env=dict(os.environ), capture_output=True, text=True, timeout=900)


def test_pseudo_label_then_self_distill_scripts(tmp_path):
    """test.py --saveres over cityscapes_train writes the labels train_src.py reads through cityscapes_self_distill_train."""
    pytest.importorskip("PIL")
    from PIL import Image
    from rnd_semantic_segmentation_amd.host import config as hc
    from rnd_semantic_segmentation_amd.host import datasets, modules
    data = tmp_path / "data"
    stems = []
    for city, n in (("aachen", 2), ("bochum", 1)):
        os.makedirs(data / "cityscapes" / "leftImg8bit" / "train" / city)
        os.makedirs(data / "cityscapes" / "gtFine" / "train" / city)
        for i in range(n):
            stem = "%s_%06d_000019" % (city, i)
            stems.append((city, stem))
            Image.fromarray(ref.synth_picture(96, 192, 300 + i)).save(str(data / "cityscapes" / "leftImg8bit" / "train" / city / (stem + "_leftImg8bit.png")))
            Image.fromarray(ref.synth_ids(96, 192, 300 + i)).save(str(data / "cityscapes" / "gtFine" / "train" / city / (stem + "_gtFine_labelIds.png")))
    fe = modules.resnet_feature_extractor("resnet101", freeze_bn=True, pretrained_backbone=False)
    cls = modules.ASPP_Classifier_V2(2048, [6, 12, 18, 24], [6, 12, 18, 24], 19)
    synth.load_formula_weights(fe)
    synth.load_formula_weights(cls)
    ckpt = str(tmp_path / "adapted.pth")
    torch.save({"feature_extractor": fe.state_dict(), "classifier": cls.state_dict()}, ckpt)
    out = str(tmp_path / "run")
    pseudo_dir = str(data / "cityscapes" / "soft_labels")
    where = ["DATASETS.DATASET_DIR", str(data), "OUTPUT_DIR", out]
    common = ["-cfg", "configs/deeplabv2_r101_self_distill.yaml"] + where
    # this process's view of the same evaluation: same checkpoint, same loader geometry
    cfg = hc.cfg.clone()
    cfg.defrost()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "deeplabv2_r101_adv_gta5.yaml"))
    cfg.merge_from_list(["DATASETS.DATASET_DIR", str(data), "DATASETS.TEST", "cityscapes_train", "INPUT.INPUT_SIZE_TEST", "(193, 97)"])
    from core.datasets.build import build_collate_fn, build_dataset
    test_set = build_dataset(cfg, mode="test", is_source=False)
    loader = datasets.wrap_loader(test_set, batch_size=1, shuffle=False, num_workers=2, pin_memory=True, collate_fn=build_collate_fn(cfg), sampler=None)
    fe, cls = fe.cuda().eval().set_precision("fp32"), cls.cuda().eval().set_precision("fp32")
    # The threshold is a test input: the median winning probability of the three images, read off the PROBABILITY kernel (the literal tail), so
    # that some pixels fall below it and some do not whatever the formula weights give (their maxima all lie under 0.9).
    tops = {}
    with torch.no_grad():
        for x, y, name in loader:
            low = cls._low_fp32(fe(x.cuda()))[0]
            tops[name[0]] = K.upsample_softmax_multi([low], [False], tuple(y.shape[-2:]), 1.0, 1.0).max(1)[0][0].cpu().numpy()
    every = np.concatenate([t.ravel() for t in tops.values()])
    threshold = round(float(np.median(every)), 4)
    assert float(every.min()) < threshold < float(every.max())
    # the labels come from the adapted model: its own configuration (frozen BatchNorm), as README's quick start runs it
    r = _run(["test.py", "--saveres", "-cfg", "configs/deeplabv2_r101_adv_gta5.yaml"] + where + ["resume", ckpt, "DATASETS.TEST", "cityscapes_train", "PSEUDO_DIR", pseudo_dir,
                                                  "INPUT.INPUT_SIZE_TEST", "(193, 97)", "TEST.PSEUDO_THRESHOLD", repr(threshold)])
    assert r.returncode == 0, r.stderr[-3000:]
    folder = os.path.join(pseudo_dir, "inference", "cityscapes_train")
    assert sorted(os.listdir(folder)) == sorted(stem + "_leftImg8bit.png" for _, stem in stems)
    distill = datasets.DatasetCatalog.get(cfg, "cityscapes_self_distill_train", "train", 19)
    assert isinstance(distill, datasets.cityscapesSelfDistillDataSet) and len(distill) == 3
    yielded = {distill[i][2]: np.asarray(distill[i][1]) for i in range(3)}
    n255 = total = 0
    for x, y, name in loader:
        r = M.predict_and_score(fe, cls, x.cuda(), y.cuda().long(), num_classes=19, threshold=threshold)
        want = r.pseudo.cpu().numpy()
        saved = np.array(Image.open(os.path.join(folder, name[0] + ".png")))
        assert np.array_equal(saved, want), name
        assert np.array_equal(want == 255, tops[name[0]] < np.float32(threshold))
        assert np.array_equal(yielded[name[0]], want.astype(np.float32))         # 0..18 kept, 255 stays 255: what the training step reads
        n255 += int((want == 255).sum())
        total += want.size
    print("self-distillation labels: %d of %d pixels below %r arrive as 255" % (n255, total, threshold))
    assert 0 < n255 < total
    r = _run(["train_src.py"] + common + ["SOLVER.EPOCHS", "1", "SOLVER.BATCH_SIZE", "2", "SOLVER.CHECKPOINT_PERIOD", "1",
                                          "INPUT.SOURCE_INPUT_SIZE_TRAIN", "(161, 129)", "INPUT.INPUT_SCALES_TRAIN", "(0.8, 1.5)"])
    assert r.returncode == 0, r.stderr[-3000:]
    assert os.path.exists(os.path.join(out, "Aspp-1.pth"))
    chart = json.load(open(os.path.join(out, "aspp_chart_params.json")))
    assert len(chart["loss"]) >= 1 and all(np.isfinite(v) for v in chart["loss"])
