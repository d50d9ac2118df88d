"""CPU tests of class weights and label smoothing in the fused cross-entropy heads: the float64 restatement (tests/_wce_ref.py) against torch's own
F.cross_entropy, the SOLVER.CLASS_WEIGHTS / SOLVER.LABEL_SMOOTHING keys, the trainers' helper (plugin.ce_options), tools/class_weights.py, and
mi_upsample_ce_w's argument checks (which return before any launch)."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import _wce_ref as R
from rnd_semantic_segmentation_amd import _lib
from rnd_semantic_segmentation_amd.host import config as hc
from rnd_semantic_segmentation_amd.host import gald, gald_fada, plugin, pranet, trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("class_weights_tool", os.path.join(ROOT, "tools", "class_weights.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("variant", R.VARIANTS, ids=lambda v: v[0])
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: s.name)
def test_restatement_is_torchs_cross_entropy(shape, variant):
    """Loss and written-out gradient against F.cross_entropy(weight=, ignore_index=, label_smoothing=) with autograd, both in float64: 1e-12 (relative
    for the loss, of the largest gradient magnitude for the gradient)."""
    _, use_w, s = variant
    low, lab, w = R.shape_inputs(shape)
    w = w if use_w else None
    r = R.wce_ref(low, lab, w, s, shape.align_corners)
    loss, d = R.wce_autograd(low, lab, w, s, shape.align_corners)
    assert r.bad == 0 and float(r.S) > 0
    assert abs(float(r.loss) - float(loss)) <= 1e-12 * max(abs(float(loss)), 1.0)
    assert (r.dlow - d).abs().max() <= 1e-12 * max(float(d.abs().max()), 1e-30)
    if shape.K == 1:
        assert float(r.loss) == 0.0 and float(r.S) == float((lab != 255).sum() * (w[0] if use_w else 1.0))


def test_restatement_edge_cases():
    shape = R.SHAPE_BY_NAME["k19_ac"]
    low, lab, w = R.shape_inputs(shape)
    assert 0.15 < (lab == 255).mean() < 0.25 and (w == 0).sum() == 1
    # the defaults are the plain cross-entropy
    r = R.wce_ref(low, lab, None, 0.0, True)
    loss, d = R.wce_autograd(low, lab, None, 0.0, True)
    assert float(r.S) == float((lab != 255).sum()) and abs(float(r.loss) - float(loss)) < 1e-13
    # out-of-range labels are left out and counted
    bad = lab.copy()
    bad.reshape(-1)[[3, 50, 51, 400]] = [19, -1, 254, 1000]
    as_ignored = lab.copy()
    as_ignored.reshape(-1)[[3, 50, 51, 400]] = 255
    a, b = R.wce_ref(low, bad, w, 0.1, True), R.wce_ref(low, as_ignored, w, 0.1, True)
    assert a.bad == 4 and b.bad == 0 and float(a.loss) == float(b.loss) and torch.equal(a.dlow, b.dlow)
    # S == 0: nan, as torch
    only_zero = np.full_like(lab, int(np.flatnonzero(w == 0)[0]))
    assert np.isnan(float(R.wce_ref(low, only_zero, w, 0.0, True).loss)) and np.isnan(float(R.wce_autograd(low, only_zero, w, 0.0, True)[0]))
    assert np.isnan(float(R.wce_ref(low, np.full_like(lab, 255), w, 0.1, True).loss))


def _cfg(*opts, yaml=None):
    c = hc.CfgNode(hc.default_tree())
    if yaml:
        c.merge_from_file(yaml)
    c.merge_from_list(list(opts))
    return c


def test_config_keys_defaults_merges_and_refusals(tmp_path):
    c = _cfg()
    assert c.SOLVER.CLASS_WEIGHTS == () and c.SOLVER.LABEL_SMOOTHING == 0.0 and isinstance(c.SOLVER.LABEL_SMOOTHING, float)
    c = _cfg("SOLVER.CLASS_WEIGHTS", "[1, 2.5, 0]", "SOLVER.LABEL_SMOOTHING", "0.1")
    assert c.SOLVER.CLASS_WEIGHTS == (1, 2.5, 0) and isinstance(c.SOLVER.CLASS_WEIGHTS, tuple) and c.SOLVER.LABEL_SMOOTHING == 0.1
    c = _cfg("SOLVER.CLASS_WEIGHTS", (0.5, 1.5), "SOLVER.LABEL_SMOOTHING", 1)
    assert c.SOLVER.CLASS_WEIGHTS == (0.5, 1.5) and c.SOLVER.LABEL_SMOOTHING == 1.0 and isinstance(c.SOLVER.LABEL_SMOOTHING, float)
    path = tmp_path / "w.yaml"
    path.write_text("SOLVER:\n  CLASS_WEIGHTS: [1.0, 2.0, 0.5]\n  LABEL_SMOOTHING: 0.05\n")
    c = _cfg(yaml=str(path))
    assert c.SOLVER.CLASS_WEIGHTS == (1.0, 2.0, 0.5) and isinstance(c.SOLVER.CLASS_WEIGHTS, tuple) and c.SOLVER.LABEL_SMOOTHING == 0.05
    for value in ("1.5", "-0.1", -1e-9, 2):
        with pytest.raises(ValueError, match="SOLVER.LABEL_SMOOTHING"):
            _cfg("SOLVER.LABEL_SMOOTHING", value)
    with pytest.raises(ValueError, match="SOLVER.LABEL_SMOOTHING"):
        _cfg("SOLVER.LABEL_SMOOTHING", "high")
    for value in ("0.5", "median", 3):
        with pytest.raises(ValueError, match="SOLVER.CLASS_WEIGHTS"):
            _cfg("SOLVER.CLASS_WEIGHTS", value)
    c = _cfg(yaml=os.path.join(ROOT, "configs", "deeplabv2_r101_src_weighted.yaml"))
    plain = _cfg(yaml=os.path.join(ROOT, "configs", "deeplabv2_r101_src.yaml"))
    assert len(c.SOLVER.CLASS_WEIGHTS) == c.MODEL.NUM_CLASSES == 19 and c.SOLVER.LABEL_SMOOTHING == 0.1 and c.SOLVER.LOSS == "ce"
    assert plain.SOLVER.CLASS_WEIGHTS == () and plain.SOLVER.LABEL_SMOOTHING == 0.0
    for k in ("MODEL", "DATASETS", "INPUT", "AUG", "TEST"):
        assert c[k] == plain[k]


TRAINERS = ("ASPPTrainer", "GALDTrainer", "PraNetTrainer", "AsppFada", "GaldFada")


@pytest.mark.parametrize("who", TRAINERS)
def test_helper_defaults(who):
    assert plugin.ce_options(_cfg(), who) == (None, 0.0)
    assert plugin.ce_options(_cfg("SOLVER.LOSS", "gdl"), who) == (None, 0.0)          # the keys at their defaults refuse nothing


def test_helper_values_and_refusals():
    w, s = plugin.ce_options(_cfg("MODEL.NUM_CLASSES", 3, "SOLVER.CLASS_WEIGHTS", "(1, 0, 2.5)", "SOLVER.LABEL_SMOOTHING", 0.1), "ASPPTrainer")
    assert w.dtype == torch.float32 and w.tolist() == [1.0, 0.0, 2.5] and s == 0.1
    w, s = plugin.ce_options(_cfg("SOLVER.LABEL_SMOOTHING", 0.2), "GALDTrainer")
    assert w is None and s == 0.2
    with pytest.raises(ValueError, match="3 entries.*NUM_CLASSES is 19"):
        plugin.ce_options(_cfg("MODEL.NUM_CLASSES", 19, "SOLVER.CLASS_WEIGHTS", "(1, 1, 1)"), "ASPPTrainer")
    with pytest.raises(ValueError, match=r"CLASS_WEIGHTS\[1\]"):
        plugin.ce_options(_cfg("MODEL.NUM_CLASSES", 3, "SOLVER.CLASS_WEIGHTS", "(1, -0.5, 1)"), "ASPPTrainer")
    for bad in (float("inf"), float("nan")):
        c = _cfg("MODEL.NUM_CLASSES", 2)
        c.SOLVER.CLASS_WEIGHTS = (1.0, bad)
        with pytest.raises(ValueError, match=r"CLASS_WEIGHTS\[1\]"):
            plugin.ce_options(c, "GALDTrainer")
    with pytest.raises(NotImplementedError, match="SOLVER.LOSS 'ce'"):
        plugin.ce_options(_cfg("MODEL.NUM_CLASSES", 19, "SOLVER.LOSS", "gdl", "SOLVER.CLASS_WEIGHTS", str((1.0,) * 19)), "GALDTrainer")
    with pytest.raises(NotImplementedError, match="structure loss"):
        plugin.ce_options(_cfg("SOLVER.LABEL_SMOOTHING", 0.1), "PraNetTrainer")


def test_trainers_use_the_helper(tmp_path):
    """Constructed on the CPU: PraNetTrainer refuses smoothing, GALDTrainer refuses weights with the Dice loss, ASPPTrainer refuses the keys on its
    unfused fallback (a classifier without .loss) instead of ignoring them, and a wrong length is refused by GaldFada through its trainer."""
    out = ["OUTPUT_DIR", str(tmp_path)]
    with pytest.raises(NotImplementedError, match="structure loss"):
        pranet.PraNetTrainer("t", _cfg("SOLVER.LABEL_SMOOTHING", 0.1, *out), None, 0)
    with pytest.raises(NotImplementedError, match="SOLVER.LOSS 'ce'"):
        gald.GALDTrainer("t", _cfg("SOLVER.LOSS", "gdl", "SOLVER.LABEL_SMOOTHING", 0.1, *out), None, 0)
    with pytest.raises(ValueError, match="3 entries.*NUM_CLASSES is 19"):
        gald_fada.GaldFada("t", _cfg("MODEL.NUM_CLASSES", 19, "SOLVER.CLASS_WEIGHTS", "(1, 2, 3)", *out), None, None, 0)

    class Foreign(trainer.ASPPTrainer):          # a classifier without .loss trains through criterion(classifier(feat, size), label)
        build_feature_extractor = staticmethod(lambda cfg: torch.nn.Conv2d(3, 4, 1))
        build_classifier = staticmethod(lambda cfg: torch.nn.Conv2d(4, 2, 1))

    with pytest.raises(NotImplementedError, match="unfused fallback"):
        Foreign("t", _cfg("SOLVER.LABEL_SMOOTHING", 0.1, *out), None, 0)
    with pytest.raises(NotImplementedError, match="unfused fallback"):
        Foreign("t", _cfg("SOLVER.CLASS_WEIGHTS", "(1, 2)", *out), None, 0)
    t = Foreign("t", _cfg(*out), None, 0)          # the defaults go through as ever
    assert t.ce_kwargs == {} and t.ce_weights is None and t.ce_smoothing == 0.0


def test_layers_refuse_what_they_cannot_honour():
    dec = gald.GCPADecoder(3)
    x, feats, lab = torch.zeros(1, 3, 8, 8), [torch.zeros(1, 1, 1, 1)] * 4, torch.zeros(1, 8, 8, dtype=torch.int64)
    with pytest.raises(ValueError, match="criterion 'ce'"):
        dec.losses(x, feats, lab, criterion="gdl", label_smoothing=0.1)
    with pytest.raises(ValueError, match="label_smoothing"):
        gald.CrossEntropyNHWC(label_smoothing=1.5)
    crit = gald.CrossEntropyNHWC(weight=[1.0, 2.0, 0.0], label_smoothing=0.1)
    assert crit.weight.dtype == torch.float32 and crit.weight.tolist() == [1.0, 2.0, 0.0] and crit.label_smoothing == 0.1
    assert gald.CrossEntropyNHWC().weight is None and gald.CrossEntropyNHWC().label_smoothing == 0.0


def test_class_weights_tool_on_a_hand_made_label_set(capsys):
    """Three images of 8 pixels, 4 classes, class 3 never seen, 255 ignored.  Class 0: 6 pixels in images 0 and 1 (16 pixels): f = 3/8; class 1: 8 pixels
    in images 0, 1, 2 (24): f = 1/3; class 2: 4 pixels in image 2 (8): f = 1/2.  median(f) = 3/8."""
    T = _tool()
    labels = [np.array([[0, 0, 0, 0], [1, 1, 255, 255]]), np.array([[0, 0, 1, 1], [1, 1, 255, 255]]), np.array([[2, 2, 2, 2], [1, 1, 255, 255]])]
    pixels, image_pixels = T.count_labels(labels, 4)
    assert pixels.tolist() == [6, 8, 4, 0] and image_pixels.tolist() == [16, 24, 8, 0]
    w = T.class_weights(pixels, image_pixels, "median")
    assert np.allclose(w, [1.0, (3 / 8) / (1 / 3), (3 / 8) / (1 / 2), 0.0], rtol=1e-15) and w[3] == 0.0
    e = T.class_weights(pixels, image_pixels, "enet")
    assert np.allclose(e[:3], [1 / np.log(1.02 + 6 / 18), 1 / np.log(1.02 + 8 / 18), 1 / np.log(1.02 + 4 / 18)], rtol=1e-15) and e[3] == 0.0
    with pytest.raises(ValueError, match="scheme"):
        T.class_weights(pixels, image_pixels, "inverse")
    assert T.format_line(w) == "SOLVER.CLASS_WEIGHTS (1.0000, 1.1250, 0.7500, 0.0000)"
    # the command line on the synthetic data: a line the configuration accepts, one weight per class
    T.main(["--scheme", "enet", "MODEL.NUM_CLASSES", "5", "INPUT.SOURCE_INPUT_SIZE_TRAIN", "(40, 24)"])
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("SOLVER.CLASS_WEIGHTS")][0]
    key, value = line.split(" ", 1)
    c = _cfg("MODEL.NUM_CLASSES", 5, key, value)
    w5, _ = plugin.ce_options(c, "ASPPTrainer")
    assert w5.shape == (5,) and bool((w5 > 0).all())


def test_cabi_argument_checks_refuse_before_any_launch():
    try:
        L = _lib.lib()
    except _lib.MiError as e:
        pytest.fail("libmi355seg.so not built: %s" % e)
    one = ctypes.c_void_p(256)          # non-null dummy: every check below fails before anything is dereferenced or launched

    def call(low=one, labels=one, cw=one, out=one, ws=one, B=2, h=5, w=7, K=19, H=20, W=28, s=0.1, gs=1.0, nbytes=1 << 30):
        return L.mi_upsample_ce_w(low, labels, cw, out, None, B, h, w, K, H, W, 255, s, gs, 0, ws, nbytes, None)

    assert call(low=None) == -22 and b"null operand" in L.mi_last_error()
    assert call(labels=None) == -22 and call(out=None) == -22
    assert call(ws=None) == -22 and b"null operand" in L.mi_last_error()
    assert call(K=33) == -22 and b"K <= 32" in L.mi_last_error()
    assert call(K=0) == -22 and call(B=0) == -22
    assert call(H=4) == -22 and b"only upsampling" in L.mi_last_error()
    assert call(s=1.5) == -22 and b"label_smoothing outside [0, 1]" in L.mi_last_error()
    assert call(s=-0.01) == -22 and b"label_smoothing outside [0, 1]" in L.mi_last_error()
    assert call(s=float("nan")) == -22 and b"not finite" in L.mi_last_error()
    assert call(s=float("inf")) == -22 and b"not finite" in L.mi_last_error()
    assert call(gs=float("nan")) == -22 and b"grad_scale" in L.mi_last_error()
    need = L.mi_upsample_ce_workspace(2, 5, 7, 19, 20, 28)
    assert call(nbytes=need - 1) != 0 and b"workspace too small" in L.mi_last_error()
    assert call(cw=None, nbytes=need - 1) != 0 and b"workspace too small" in L.mi_last_error()          # NULL weights pass the operand check
