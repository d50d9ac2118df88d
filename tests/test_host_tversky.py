"""CPU tests of the Tversky + BCE loss's host side: the float64 restatement (tests/_tversky_ref.py) against the reference's own results
(tests/golden/g17_tversky.npz, written by tools/make_golden_tversky.py), the SOLVER.LOSS / SOLVER.TVERSKY_ALPHA keys, the drop-in import path, the
refusals of the loss modules and of the trainers that do not implement it, and mi_upsample_tversky_bce's argument checks (which return before any
launch)."""
import ctypes
import hashlib
import os

import numpy as np
import pytest
import torch

import _tversky_ref as T
from rnd_semantic_segmentation_amd import _lib
from rnd_semantic_segmentation_amd.host import config as hc
from rnd_semantic_segmentation_amd.host import gald, gald_fada, losses, pranet, trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS_BAR, GRAD_BAR = 2e-5, 2e-5          # the project's bars for fused upsample losses (tests/test_gpu_ops.py, tests/test_gpu_gdl.py)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "g17_tversky.npz"))


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.name)
def test_restatement_reproduces_the_reference(golden, case):
    """The reference's own fp32 run sits at 6e-8 relative on the loss and 1.4e-6 of the largest |dlow| against float64; asserted at the project's bars:
    loss and its two terms 2e-5 relative, dlow 2e-5 of the reference's largest |dlow|."""
    low, mask = T.case_inputs(case)
    assert str(golden[case.name + ".in_sha"]) == _sha(low) + _sha(mask)
    r = T.tversky_ref(low, mask, case.align_corners)
    want_d = golden[case.name + ".dlow"].astype(np.float64)
    for got, key in ((r.loss, ".loss"), (r.tversky, ".tversky"), (r.bce, ".bce")):
        want = float(golden[case.name + key])
        err = abs(float(got) - want) / abs(want)
        print("%s%s: %.9g vs %.9g, %.3e rel" % (case.name, key, float(got), want, err))
        assert np.isfinite(want) and err < LOSS_BAR, (key, err)
    e_d = np.abs(r.dlow.numpy() - want_d).max() / np.abs(want_d).max()
    print("%s: dlow %.3e relmax, |dlow|max %.3e" % (case.name, e_d, np.abs(want_d).max()))
    assert np.isfinite(want_d).all() and np.abs(want_d).max() > 1e-3 and e_d < GRAD_BAR, e_d
    if case.mask == "zero":
        assert float(r.TP) == 0.0 and float(r.FN) == 0.0 and float(r.FP) > 0.0
    if case.mask == "one":
        assert float(r.FP) == 0.0 and float(r.TP) > 0.0
    if case.sat:
        assert np.abs(low).max() == np.float32(80.0) and float(golden[case.name + ".loss"]) > 2.0


@pytest.mark.parametrize("name,alpha,weights", [("a", 0.7, (0.5, 0.5)), ("c", 0.3, (1.0, 0.0)), ("g", 0.7, (0.0, 1.0)), ("i", 1.0, (0.25, 0.75)),
                                                ("h", 0.0, (0.5, 0.5))])
def test_written_out_gradient_is_the_autograd_gradient(name, alpha, weights):
    case = T.CASE_BY_NAME[name]
    low, mask = T.case_inputs(case)
    r = T.tversky_ref(low, mask, case.align_corners, alpha=alpha, weights=weights)
    loss, d = T.tversky_autograd(low, mask, case.align_corners, alpha=alpha, weights=weights)
    assert abs(float(r.loss) - float(loss)) < 1e-13 * max(1.0, abs(float(loss)))
    assert (r.dlow - d).abs().max() < 1e-10 * d.abs().max()


def _cfg(*opts, yaml=None):
    c = hc.CfgNode(hc.default_tree())
    if yaml:
        c.merge_from_file(yaml)
    c.merge_from_list(list(opts))
    return c


def test_config_keys_merge_and_refuse_other_values(tmp_path):
    c = _cfg()
    assert c.SOLVER.LOSS == "ce" and c.SOLVER.TVERSKY_ALPHA == 0.7
    c = _cfg("SOLVER.LOSS", "tversky", "SOLVER.TVERSKY_ALPHA", "0.3")
    assert c.SOLVER.LOSS == "tversky" and c.SOLVER.TVERSKY_ALPHA == 0.3
    assert _cfg("SOLVER.TVERSKY_ALPHA", 1).SOLVER.TVERSKY_ALPHA == 1.0 and _cfg("SOLVER.TVERSKY_ALPHA", 0.0).SOLVER.TVERSKY_ALPHA == 0.0
    for key, value in (("SOLVER.LOSS", "Tversky"), ("SOLVER.LOSS", "dice"), ("SOLVER.TVERSKY_ALPHA", 1.5), ("SOLVER.TVERSKY_ALPHA", "-0.1")):
        with pytest.raises(ValueError, match=key):
            _cfg(key, value)
    path = tmp_path / "bad.yaml"
    path.write_text("SOLVER:\n  TVERSKY_ALPHA: 1.5\n")
    with pytest.raises(ValueError, match="SOLVER.TVERSKY_ALPHA"):
        _cfg(yaml=str(path))


def test_the_yaml_loads():
    c = _cfg(yaml=os.path.join(ROOT, "configs", "pranet_src_polyp_tversky.yaml"))
    assert c.SOLVER.LOSS == "tversky" and c.SOLVER.TVERSKY_ALPHA == 0.7 and c.SOLVER.BATCH_SIZE == 16 and c.INPUT.TRAINSIZE == 352
    plain = _cfg(yaml=os.path.join(ROOT, "configs", "pranet_src_polyp.yaml"))
    assert plain.SOLVER.LOSS == "ce"
    for k in ("MODEL", "DATASETS", "INPUT", "TEST"):
        assert c[k] == plain[k]


def test_dropin_import_identity():
    from core.models.classifiers.attn.loss import BinaryCrossEntropyLoss, CompoundLoss, MultiscaleLoss, TverskyLoss
    assert TverskyLoss is losses.TverskyLoss and BinaryCrossEntropyLoss is losses.BinaryCrossEntropyLoss
    assert CompoundLoss is losses.CompoundLoss and MultiscaleLoss is losses.MultiscaleLoss
    t = TverskyLoss()
    assert t.alpha == 0.7 and t.eps == 1
    c = CompoundLoss([TverskyLoss(0.3, 2), BinaryCrossEntropyLoss(), BinaryCrossEntropyLoss()])
    assert c.weights == [1. / 3] * 3 and len(c.losses) == 3 and c.losses[0].alpha == 0.3 and c.losses[0].eps == 2
    assert CompoundLoss([t], weights=[2.0]).weights == [2.0]
    assert MultiscaleLoss(c).loss_fn is c
    for name in ("core.models.classifiers.attn.attn", "core.models.classifiers.attn.efficientnet", "core.trainers.attn_trainer"):
        with pytest.raises(ImportError, match="not part of the MI355X hot path"):
            __import__(name)


def test_loss_modules_refuse_cpu_tensors_and_several_channels():
    pred, lab = torch.zeros(2, 1, 4, 5), torch.zeros(2, 1, 4, 5)
    for crit in (losses.TverskyLoss(), losses.BinaryCrossEntropyLoss(), losses.CompoundLoss([losses.TverskyLoss(), losses.BinaryCrossEntropyLoss()]),
                 losses.MultiscaleLoss(losses.TverskyLoss())):
        args = ([pred], [lab]) if isinstance(crit, losses.MultiscaleLoss) else (pred, lab)
        with pytest.raises(NotImplementedError, match="MI355X only"):
            crit(*args)


def test_several_channels_are_refused_by_name(monkeypatch):
    """C > 1 is refused with its own message (the device check is taken out of the way: no GPU here)."""
    class Fake:
        is_cuda, device = True, "cuda:0"

        def __init__(self, *shape):
            self.shape = shape

        def dim(self):
            return len(self.shape)
    with pytest.raises(NotImplementedError, match="C > 1"):
        losses.tversky_bce(Fake(2, 3, 4, 5), Fake(2, 3, 4, 5))
    with pytest.raises(ValueError, match="does not match"):
        losses.tversky_bce(Fake(2, 1, 4, 5), Fake(2, 1, 4, 6))
    with pytest.raises(ValueError, match="alpha"):
        losses.tversky_bce(Fake(2, 1, 4, 5), Fake(2, 1, 4, 5), alpha=1.5)


@pytest.mark.parametrize("make", [
    lambda c: trainer.ASPPTrainer("t", c, None, 0),
    lambda c: gald.GALDTrainer("t", c, None, 0),
    lambda c: gald_fada.GaldFada("t", c, None, None, 0),
], ids=["ASPPTrainer", "GALDTrainer", "GaldFada"])
def test_other_trainers_refuse_the_tversky_loss(tmp_path, make):
    c = _cfg("SOLVER.LOSS", "tversky", "OUTPUT_DIR", str(tmp_path))
    with pytest.raises(NotImplementedError, match="PraNetTrainer"):
        make(c)
    assert pranet.PraNetTrainer.LOSSES == ("ce", "tversky") and gald.GALDTrainer.LOSSES == ("ce", "gdl")


def test_pranet_trainer_still_refuses_the_dice_loss(tmp_path):
    c = _cfg("SOLVER.LOSS", "gdl", "OUTPUT_DIR", str(tmp_path))
    with pytest.raises(NotImplementedError, match="GALDTrainer"):
        pranet.PraNetTrainer("t", c, None, 0)


def test_pranet_losses_refuses_bad_arguments():
    net = pranet.PraNet()
    x, gt = torch.zeros(1, 3, 32, 32), torch.zeros(1, 1, 32, 32)
    with pytest.raises(ValueError, match="alpha"):
        net.losses(x, gt, alpha=1.5)
    with pytest.raises(ValueError, match="alpha"):
        net.losses(x, gt, eps=0.0)
    with pytest.raises(ValueError, match="gts must be"):
        net.losses(x, torch.zeros(1, 2, 32, 32))
    with pytest.raises(ValueError, match="gts must be"):
        net.losses(x, torch.zeros(1, 1, 16, 32))
    with pytest.raises(ValueError, match="criterion"):
        pranet.step_losses(net, x, gt, criterion="gdl")
    assert net.__dict__.get("_tversky") is None


def test_cabi_argument_checks_refuse_before_any_launch():
    try:
        L = _lib.lib()
    except _lib.MiError as e:
        pytest.fail("libmi355seg.so not built: %s" % e)
    one = ctypes.c_void_p(256)          # non-null dummy: every check below fails before anything is dereferenced or launched

    def call(low=one, mask=one, out=one, ws=one, B=2, h=5, w=7, H=20, W=28, alpha=0.7, eps=1.0, nbytes=1 << 30):
        return L.mi_upsample_tversky_bce(low, mask, out, None, None, B, h, w, H, W, alpha, eps, 0.5, 0.5, 1.0, 0, ws, nbytes, None)

    for kw in (dict(low=None), dict(mask=None), dict(out=None), dict(ws=None)):
        assert call(**kw) == -22 and b"null operand" in L.mi_last_error(), kw
    assert call(B=0) == -22 and call(w=0) == -22 and b"bad dimension" in L.mi_last_error()
    assert call(H=4) == -22 and b"only upsampling" in L.mi_last_error()
    assert call(W=6) == -22 and b"only upsampling" in L.mi_last_error()
    assert call(alpha=1.5) == -22 and b"alpha" in L.mi_last_error()
    assert call(alpha=-0.01) == -22 and call(alpha=float("nan")) == -22 and b"alpha" in L.mi_last_error()
    assert call(eps=0.0) == -22 and b"eps" in L.mi_last_error()
    assert call(eps=-1.0) == -22
    need = L.mi_upsample_tversky_bce_workspace(2, 5, 7, 20, 28)
    assert need >= 2 * 20 * 7 * 4 + 3 * 4 + 4 * 4
    assert call(nbytes=need - 1) != 0 and b"workspace too small" in L.mi_last_error()
    assert L.mi_upsample_tversky_bce_workspace(0, 5, 7, 20, 28) == 0
