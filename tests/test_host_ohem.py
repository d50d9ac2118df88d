"""CPU tests of online hard example mining (OHEM) in the fused cross-entropy heads: the float64 restatement (tests/_ohem_ref.py) against
F.cross_entropy on the kept pixels, the margin condition every parity case of tests/test_gpu_ohem.py has to meet, the SOLVER.LOSS "ohem" /
SOLVER.OHEM_THRESH / SOLVER.OHEM_MIN_KEPT keys, the trainers' helper (plugin.ohem_options), the refusals of the layers, and mi_upsample_ce_ohem's
argument checks (which return before any launch)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _ohem_ref as R
from rnd_semantic_segmentation_amd import _lib, kernels
from rnd_semantic_segmentation_amd.host import config as hc
from rnd_semantic_segmentation_amd.host import fada, gald, gald_fada, modules, plugin, pranet, trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c.name for c in R.CASES]


def test_the_case_table_is_the_one_the_issue_sets():
    assert len(R.CASES) == 10 * 3 + 4 and len(set(NAMES)) == len(NAMES)
    for g in R.GEOMETRY:
        n = {s: int((R.case_inputs("%s-%s" % (g, s))[1] != 255).sum()) for s in ("minkept", "all")}          # (a salted case has its own labels)
        assert R.case_inputs(g + "-minkept")[2:] == (0.05, max(1, n["minkept"] // 3))
        assert R.case_inputs(g + "-thresh")[2:] == (0.7, 1)
        assert R.case_inputs(g + "-all")[3] == 10 * n["all"]
    low, lab, _, _ = R.case_inputs("cluster")
    assert np.abs(low).max() == np.float32(1e-3)
    assert R.MANY_WG.B * R.MANY_WG.HW[0] * R.MANY_WG.HW[1] > 16 * 256 and R.SECOND_TRIP.HW[0] * R.SECOND_TRIP.HW[1] > 1024 * 256


@pytest.mark.parametrize("name", NAMES)
def test_restatement_is_cross_entropy_over_the_kept_pixels(name):
    """Loss and written-out gradient against F.cross_entropy(z, where(kept, label, ignore)) with autograd, both in float64: 1e-12."""
    low, lab, thresh, min_kept = R.case_inputs(name)
    r = R.case_ref(name)
    loss, d = R.ohem_autograd(low, lab, r.kept, R.CASE_BY_NAME[name].shape.align_corners)
    n = int((lab != 255).sum())
    assert r.bad == 0 and r.n_kept >= min(min_kept, n) >= 1 and r.t >= thresh
    assert abs(float(r.loss) - float(loss)) <= 1e-12 * max(abs(float(loss)), 1.0)
    assert (r.dlow - d).abs().max() <= 1e-12 * max(float(d.abs().max()), 1e-30)


@pytest.mark.parametrize("name", NAMES)
def test_margin_condition(name):
    """No valid pixel's q lies within a relative 1e-4 of t without being t: a kernel inside its 2e-5 bar keeps the same pixels as float64 does.  A
    condition on the inputs: a case that misses it gets another salt in _ohem_ref._SALTS."""
    r = R.case_ref(name)
    print("%s: margin %.3e, t %.6g, n_kept %d" % (name, r.margin, r.t, r.n_kept))
    if name == "ties":          # every q is equal: all are t
        n = int((R.case_inputs(name)[1] != 255).sum())
        assert r.margin == float("inf") and r.n_kept == n and abs(r.t - 1.0 / 19.0) < 1e-15
        return
    assert r.margin >= R.MARGIN


def test_what_decides_in_the_settings():
    k19 = R.case_ref("k19-all")
    low, lab, _, _ = R.case_inputs("k19-all")
    n = int((lab != 255).sum())
    assert k19.n_kept == n                                                          # min_kept >= n: the plain cross-entropy
    assert R.case_ref("k19-thresh").t == 0.7 and R.case_ref("many_wg").t > 0.001          # thresh decides / min_kept decides
    mk = R.case_inputs("many_wg")[3]
    assert R.case_ref("many_wg").n_kept == mk and R.case_ref("second_trip").n_kept == 64
    c = R.case_ref("cluster")
    q = c.q[c.q < 1.5]
    assert float((q.max() - q.min()) / q.min()) < 2e-3          # all q share their leading bits: the last radix level decides


def test_restatement_edge_cases():
    low, lab, _, _ = R.case_inputs("k19_ac-all")
    # every pixel ignored: nan, nothing kept, t = thresh
    r = R.ohem_ref(low, np.full_like(lab, 255), 0.3, 10, True)
    assert np.isnan(float(r.loss)) and r.n_kept == 0 and r.t == 0.3 and not r.dlow.any()
    # out-of-range labels are left out and counted
    bad = lab.copy()
    bad.reshape(-1)[[3, 50, 51, 400]] = [19, -1, 254, 1000]
    as_ignored = lab.copy()
    as_ignored.reshape(-1)[[3, 50, 51, 400]] = 255
    a, b = R.ohem_ref(low, bad, 0.05, 500, True), R.ohem_ref(low, as_ignored, 0.05, 500, True)
    assert a.bad == 4 and b.bad == 0 and float(a.loss) == float(b.loss) and torch.equal(a.dlow, b.dlow)
    # min_kept 1, thresh 0: the pixels tied for the minimum
    r = R.ohem_ref(low, lab, 0.0, 1, True)
    assert r.n_kept == 1 and r.t == float(r.q.min())


def _cfg(*opts, yaml=None):
    c = hc.CfgNode(hc.default_tree())
    if yaml:
        c.merge_from_file(yaml)
    c.merge_from_list(list(opts))
    return c


def test_config_keys_defaults_merges_and_refusals(tmp_path):
    c = _cfg()
    assert c.SOLVER.OHEM_THRESH == 0.7 and c.SOLVER.OHEM_MIN_KEPT == 100000 and isinstance(c.SOLVER.OHEM_MIN_KEPT, int) and c.SOLVER.LOSS == "ce"
    c = _cfg("SOLVER.LOSS", "ohem", "SOLVER.OHEM_THRESH", "0.9", "SOLVER.OHEM_MIN_KEPT", "5000")
    assert (c.SOLVER.LOSS, c.SOLVER.OHEM_THRESH, c.SOLVER.OHEM_MIN_KEPT) == ("ohem", 0.9, 5000)
    path = tmp_path / "o.yaml"
    path.write_text("SOLVER:\n  LOSS: ohem\n  OHEM_THRESH: 0.6\n  OHEM_MIN_KEPT: 1\n")
    c = _cfg(yaml=str(path))
    assert (c.SOLVER.LOSS, c.SOLVER.OHEM_THRESH, c.SOLVER.OHEM_MIN_KEPT) == ("ohem", 0.6, 1)
    for value in ("1.5", "-0.1", -1e-9, 2):
        with pytest.raises(ValueError, match="SOLVER.OHEM_THRESH"):
            _cfg("SOLVER.OHEM_THRESH", value)
    for value in (0, "-5", "0", "many", 2.5):
        with pytest.raises(ValueError, match="SOLVER.OHEM_MIN_KEPT"):
            _cfg("SOLVER.OHEM_MIN_KEPT", value)
    with pytest.raises(ValueError, match="SOLVER.LOSS"):
        _cfg("SOLVER.LOSS", "hard")
    for name, plain in (("deeplabv2_r101_src_ohem.yaml", "deeplabv2_r101_src.yaml"), ("gald_src_ohem.yaml", "gald_src.yaml")):
        c, p = _cfg(yaml=os.path.join(ROOT, "configs", name)), _cfg(yaml=os.path.join(ROOT, "configs", plain))
        assert (c.SOLVER.LOSS, c.SOLVER.OHEM_THRESH, c.SOLVER.OHEM_MIN_KEPT) == ("ohem", 0.7, 100000) and p.SOLVER.LOSS == "ce"
        for k in ("MODEL", "DATASETS", "INPUT", "AUG", "TEST"):
            assert c[k] == p[k]


TRAINERS = ("ASPPTrainer", "GALDTrainer", "PraNetTrainer", "AsppFada", "GaldFada")


@pytest.mark.parametrize("who", TRAINERS)
def test_helper_defaults_and_the_keys_set_without_ohem(who):
    assert plugin.ohem_options(_cfg(), who) is None
    assert plugin.ohem_options(_cfg("SOLVER.LOSS", "gdl"), who) is None          # the keys at their defaults refuse nothing
    assert plugin.ohem_options(_cfg("SOLVER.LOSS", "ohem"), who) == (0.7, 100000)
    assert plugin.ohem_options(_cfg("SOLVER.LOSS", "ohem", "SOLVER.OHEM_THRESH", 0.5, "SOLVER.OHEM_MIN_KEPT", 7), who) == (0.5, 7)
    for opts in (("SOLVER.OHEM_THRESH", 0.5), ("SOLVER.OHEM_MIN_KEPT", 7), ("SOLVER.LOSS", "gdl", "SOLVER.OHEM_MIN_KEPT", 7)):
        with pytest.raises(NotImplementedError, match="belong to SOLVER.LOSS 'ohem'"):
            plugin.ohem_options(_cfg(*opts), who)
    c = _cfg("SOLVER.LOSS", "ohem")
    c.SOLVER.OHEM_THRESH = 1.5          # assigned, not merged
    with pytest.raises(ValueError, match="OHEM_THRESH"):
        plugin.ohem_options(c, who)
    c = _cfg("SOLVER.LOSS", "ohem")
    c.SOLVER.OHEM_MIN_KEPT = 0
    with pytest.raises(ValueError, match="OHEM_MIN_KEPT"):
        plugin.ohem_options(c, who)


def test_ohem_with_weights_or_smoothing_is_refused_by_the_helper():
    for opts in (("SOLVER.LABEL_SMOOTHING", 0.1), ("SOLVER.CLASS_WEIGHTS", str((1.0,) * 19))):
        with pytest.raises(NotImplementedError, match="'ohem' cannot be combined with SOLVER.CLASS_WEIGHTS / SOLVER.LABEL_SMOOTHING"):
            plugin.ce_options(_cfg("MODEL.NUM_CLASSES", 19, "SOLVER.LOSS", "ohem", *opts), "GALDTrainer")


def test_trainers_losses_and_refusals(tmp_path):
    """Constructed on the CPU.  ASPPTrainer and GALDTrainer know "ohem"; PraNetTrainer and both FADA combos refuse it and say where it lives; a
    trainer refuses the keys without the loss, and the loss with weights or smoothing."""
    out = ["OUTPUT_DIR", str(tmp_path)]
    # "ohem" is the cross-entropy over mined pixels: it is listed in MINED beside LOSSES, whose tuples earlier suites pin
    assert trainer.ASPPTrainer.LOSSES + trainer.ASPPTrainer.MINED == ("ce", "ohem")
    assert gald.GALDTrainer.LOSSES + gald.GALDTrainer.MINED == ("ce", "gdl", "ohem")
    assert pranet.PraNetTrainer.LOSSES + pranet.PraNetTrainer.MINED == ("ce", "tversky") and plugin.BaseTrainer.MINED == ()
    ohem = _cfg("SOLVER.LOSS", "ohem", *out)
    with pytest.raises(NotImplementedError, match="PraNetTrainer trains with.*wired into the fused cross-entropy heads of ASPPTrainer"):
        pranet.PraNetTrainer("t", ohem, None, 0)
    with pytest.raises(NotImplementedError, match="AsppFada trains with SOLVER.LOSS 'ce' only.*ASPPTrainer"):
        fada.AsppFada("t", ohem, None, None, 0)
    with pytest.raises(NotImplementedError, match="GaldFada trains with SOLVER.LOSS 'ce' only.*GALDTrainer"):
        gald_fada.GaldFada("t", ohem, None, None, 0)
    with pytest.raises(NotImplementedError, match="belong to SOLVER.LOSS 'ohem'"):
        gald.GALDTrainer("t", _cfg("SOLVER.OHEM_MIN_KEPT", 5, *out), None, 0)
    with pytest.raises(NotImplementedError, match="belong to SOLVER.LOSS 'ohem'"):
        pranet.PraNetTrainer("t", _cfg("SOLVER.OHEM_THRESH", 0.5, *out), None, 0)
    with pytest.raises(NotImplementedError, match="'ohem' cannot be combined"):
        gald.GALDTrainer("t", _cfg("SOLVER.LOSS", "ohem", "SOLVER.LABEL_SMOOTHING", 0.1, *out), None, 0)

    class Foreign(trainer.ASPPTrainer):          # a classifier without .loss trains through criterion(classifier(feat, size), label)
        build_feature_extractor = staticmethod(lambda cfg: torch.nn.Conv2d(3, 4, 1))
        build_classifier = staticmethod(lambda cfg: torch.nn.Conv2d(4, 2, 1))

    with pytest.raises(NotImplementedError, match="'ohem' cannot be combined"):
        Foreign("t", _cfg("SOLVER.LOSS", "ohem", "SOLVER.CLASS_WEIGHTS", "(1, 2)", "MODEL.NUM_CLASSES", 2, *out), None, 0)
    with pytest.raises(NotImplementedError, match="SOLVER.LOSS 'ohem'.*unfused fallback"):
        Foreign("t", ohem, None, 0)
    t = Foreign("t", _cfg(*out), None, 0)          # the defaults go through as ever
    assert t.ce_kwargs == {} and t.ohem is None


def test_layers_refuse_what_they_cannot_honour():
    dec = gald.GCPADecoder(3)
    x, feats, lab = torch.zeros(1, 3, 8, 8), [torch.zeros(1, 1, 1, 1)] * 4, torch.zeros(1, 8, 8, dtype=torch.int64)
    both = "ohem .*cannot be combined with class_weights / label_smoothing"
    with pytest.raises(NotImplementedError, match=both):
        dec.losses(x, feats, lab, criterion="ohem", ohem=(0.7, 10), label_smoothing=0.1)
    with pytest.raises(NotImplementedError, match=both):
        dec.loss(x, feats, lab, ohem=(0.7, 10), class_weights=torch.ones(3))
    with pytest.raises(ValueError, match="go together"):
        dec.losses(x, feats, lab, criterion="ohem")
    with pytest.raises(ValueError, match="go together"):
        dec.losses(x, feats, lab, criterion="ce", ohem=(0.7, 10))
    with pytest.raises(ValueError, match="thresh"):
        dec.losses(x, feats, lab, criterion="ohem", ohem=(1.5, 10))
    with pytest.raises(ValueError, match="min_kept"):
        dec.loss(x, feats, lab, ohem=(0.5, 0))
    cls = modules.ASPP_Classifier_V2(64, [6, 12, 18, 24], [6, 12, 18, 24], 3)
    with pytest.raises(NotImplementedError, match=both):
        cls.loss(torch.zeros(1, 64, 4, 4), lab, ohem=(0.7, 10), label_smoothing=0.1)
    with pytest.raises(NotImplementedError, match=both):
        cls.loss(torch.zeros(1, 64, 4, 4), lab, ohem=(0.7, 10), class_weights=torch.ones(3))
    assert kernels.check_ohem((0.7, 100000)) == (0.7, 100000) and kernels.check_ohem([0, 1]) == (0.0, 1)
    for bad in ((0.7,), 0.7, (0.7, 1.5), (-0.1, 5), (float("nan"), 5)):
        with pytest.raises(ValueError, match="ohem"):
            kernels.check_ohem(bad)


def test_cabi_argument_checks_refuse_before_any_launch():
    try:
        L = _lib.lib()
    except _lib.MiError as e:
        pytest.fail("libmi355seg.so not built: %s" % e)
    one = ctypes.c_void_p(256)          # non-null dummy: every check below fails before anything is dereferenced or launched

    def call(low=one, labels=one, out=one, ws=one, B=2, h=5, w=7, K=19, H=20, W=28, thresh=0.7, min_kept=100, gs=1.0, nbytes=1 << 30):
        return L.mi_upsample_ce_ohem(low, labels, out, None, None, B, h, w, K, H, W, 255, thresh, min_kept, gs, 0, ws, nbytes, None)

    assert call(low=None) == -22 and b"null operand" in L.mi_last_error()
    assert call(labels=None) == -22 and call(out=None) == -22
    assert call(ws=None) == -22 and b"null operand" in L.mi_last_error()
    assert call(K=33) == -22 and b"K <= 32" in L.mi_last_error()
    assert call(K=0) == -22 and call(B=0) == -22
    assert call(H=4) == -22 and b"only upsampling" in L.mi_last_error()
    assert call(B=4, H=2048, W=2048) == -22 and b"below 2^24" in L.mi_last_error()
    assert call(thresh=1.5) == -22 and b"thresh outside [0, 1]" in L.mi_last_error()
    assert call(thresh=-0.01) == -22 and b"thresh outside [0, 1]" in L.mi_last_error()
    assert call(thresh=float("nan")) == -22 and b"thresh outside [0, 1]" in L.mi_last_error()
    assert call(min_kept=0) == -22 and b"min_kept" in L.mi_last_error()
    assert call(min_kept=-(2 ** 40)) == -22 and b"min_kept" in L.mi_last_error()
    assert call(gs=float("nan")) == -22 and b"grad_scale" in L.mi_last_error()
    need = L.mi_upsample_ce_ohem_workspace(2, 5, 7, 19, 20, 28)
    assert need >= 2 * 2 * 20 * 28 * 4 + 2 * 20 * 7 * 19 * 4
    assert call(nbytes=need - 1) != 0 and b"workspace too small" in L.mi_last_error()
    assert call(min_kept=2 ** 40, nbytes=need - 1) != 0 and b"workspace too small" in L.mi_last_error()          # a min_kept above any n passes its check
