"""CPU tests of the generalized Dice loss's host side: the float64 restatement (tests/_gdl_ref.py) against the reference's own results
(tests/golden/g16_gdl.npz, written by tools/make_golden_gdl.py), the SOLVER.LOSS / SOLVER.GDL_WEIGHT keys, the drop-in import path, the refusals of the
trainers that keep cross-entropy, and mi_upsample_gdl's argument checks (which return before any launch)."""
import ctypes
import hashlib
import os

import numpy as np
import pytest
import torch

import _gdl_ref as G
from rnd_semantic_segmentation_amd import _lib
from rnd_semantic_segmentation_amd.host import config as hc
from rnd_semantic_segmentation_amd.host import gald, gald_fada, metrics, pranet, trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "g16_gdl.npz"))


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: c.name)
def test_restatement_reproduces_the_reference(golden, case):
    """Bars (the reference's own fp32 run sits at 5e-8 absolute on the loss and 1.5e-6 relmax on the gradient against float64): loss 2e-6 relative,
    dlow 2e-5 of the reference's largest |dlow|; every pixel ignored: exactly 1 and 0 on both sides."""
    low, lab = G.case_inputs(case)
    assert str(golden[case.name + ".in_sha"]) == _sha(low) + _sha(lab)
    r = G.gdl_ref(low, lab, case.align_corners, case.weight_type)
    want_loss, want_d = float(golden[case.name + ".loss"]), golden[case.name + ".dlow"].astype(np.float64)
    if case.name == "f":
        assert float(r.loss) == 1.0 and want_loss == 1.0
        assert not r.dlow.any() and not want_d.any()
        return
    e_loss = abs(float(r.loss) - want_loss) / abs(want_loss)
    e_d = np.abs(r.dlow.numpy() - want_d).max() / np.abs(want_d).max()
    print("%s: loss %.3e rel, dlow %.3e relmax" % (case.name, e_loss, e_d))
    assert e_loss < 2e-6 and e_d < 2e-5, (e_loss, e_d)
    if case.name == "c":          # the absent-class regime: weight 1 / eps dominates the denominator
        assert float(r.loss) > 1 - 1e-6 and np.abs(want_d).max() < 1e-10 and int((r.T == 0).sum()) == 14


@pytest.mark.parametrize("name", ["a_sqrt", "b_identity", "c", "e_ac"])
def test_written_out_gradient_is_the_autograd_gradient(name):
    case = G.CASE_BY_NAME[name]
    low, lab = G.case_inputs(case)
    r = G.gdl_ref(low, lab, case.align_corners, case.weight_type)
    loss, d = G.gdl_autograd(low, lab, case.align_corners, case.weight_type)
    assert abs(float(r.loss) - float(loss)) < 1e-14
    assert (r.dlow - d).abs().max() < 1e-10 * d.abs().max()


def test_restatement_leaves_out_and_counts_bad_labels():
    case = G.CASE_BY_NAME["a_square"]
    low, lab = G.case_inputs(case)
    bad = lab.copy()
    bad.reshape(-1)[[3, 50, 51, 400, 999]] = [2, 7, -1, 254, 1000]
    as_ignored = lab.copy()
    as_ignored.reshape(-1)[[3, 50, 51, 400, 999]] = 255
    r, q = G.gdl_ref(low, bad, False), G.gdl_ref(low, as_ignored, False)
    assert r.bad == 5 and q.bad == 0 and r.valid == q.valid
    assert float(r.loss) == float(q.loss) and torch.equal(r.dlow, q.dlow)


def _cfg(*opts, yaml=None):
    c = hc.CfgNode(hc.default_tree())
    if yaml:
        c.merge_from_file(yaml)
    c.merge_from_list(list(opts))
    return c


def test_config_keys_merge_and_refuse_other_values(tmp_path):
    c = _cfg()
    assert c.SOLVER.LOSS == "ce" and c.SOLVER.GDL_WEIGHT == "square"
    c = _cfg("SOLVER.LOSS", "gdl", "SOLVER.GDL_WEIGHT", "sqrt")
    assert c.SOLVER.LOSS == "gdl" and c.SOLVER.GDL_WEIGHT == "sqrt"
    c = _cfg(yaml=os.path.join(ROOT, "configs", "gald_src_dice.yaml"))
    assert c.SOLVER.LOSS == "gdl" and c.SOLVER.GDL_WEIGHT == "square" and c.SOLVER.BATCH_SIZE == 6 and c.AUG.NAME == "gald"
    plain = _cfg(yaml=os.path.join(ROOT, "configs", "gald_src.yaml"))
    assert plain.SOLVER.LOSS == "ce"
    for key, value in (("SOLVER.LOSS", "dice"), ("SOLVER.LOSS", "CE"), ("SOLVER.GDL_WEIGHT", "cube"), ("SOLVER.GDL_WEIGHT", "None"), ("SOLVER.LOSS", "1")):
        with pytest.raises(ValueError, match=key):
            _cfg(key, value)
    path = tmp_path / "bad.yaml"
    path.write_text("SOLVER:\n  LOSS: focal\n")
    with pytest.raises(ValueError, match="SOLVER.LOSS"):
        _cfg(yaml=str(path))


def test_dropin_import_and_refusals():
    from core.utils.utility import GeneralizedDiceLoss
    assert GeneralizedDiceLoss is metrics.GeneralizedDiceLoss
    out, lab = torch.zeros(2, 3, 4, 5), torch.zeros(2, 4, 5, dtype=torch.int64)
    with pytest.raises(NotImplementedError, match="MI355X only"):
        GeneralizedDiceLoss(out, lab)
    with pytest.raises(NotImplementedError, match="one-hot"):
        GeneralizedDiceLoss(out, torch.zeros(2, 3, 4, 5))
    with pytest.raises(ValueError, match="weight_type"):
        GeneralizedDiceLoss(out, lab, weight_type="cube")


@pytest.mark.parametrize("make", [
    lambda c: trainer.ASPPTrainer("t", c, None, 0),
    lambda c: pranet.PraNetTrainer("t", c, None, 0),
    lambda c: gald_fada.GaldFada("t", c, None, None, 0),
], ids=["ASPPTrainer", "PraNetTrainer", "GaldFada"])
def test_other_trainers_refuse_the_dice_loss(tmp_path, make):
    c = _cfg("SOLVER.LOSS", "gdl", "OUTPUT_DIR", str(tmp_path))
    with pytest.raises(NotImplementedError, match="GALDTrainer"):
        make(c)
    assert gald.GALDTrainer.LOSSES == ("ce", "gdl")


def test_decoder_losses_refuses_unknown_criteria():
    dec = gald.GCPADecoder(3)
    x, feats, lab = torch.zeros(1, 3, 8, 8), [torch.zeros(1, 1, 1, 1)] * 4, torch.zeros(1, 8, 8, dtype=torch.int64)
    with pytest.raises(ValueError, match="criterion"):
        dec.losses(x, feats, lab, criterion="dice")
    with pytest.raises(ValueError, match="weight_type"):
        dec.losses(x, feats, lab, criterion="gdl", weight_type="cube")


def test_cabi_argument_checks_refuse_before_any_launch():
    try:
        L = _lib.lib()
    except _lib.MiError as e:
        pytest.fail("libmi355seg.so not built: %s" % e)
    one = ctypes.c_void_p(256)          # non-null dummy: every check below fails before anything is dereferenced or launched

    def call(low=one, labels=one, out=one, ws=one, B=2, h=5, w=7, K=19, H=20, W=28, wt=0, eps=1e-5, nbytes=1 << 30):
        return L.mi_upsample_gdl(low, labels, out, None, None, B, h, w, K, H, W, 255, wt, eps, 1.0, 0, ws, nbytes, None)

    assert call(low=None) == -22 and b"null operand" in L.mi_last_error()
    assert call(ws=None) == -22 and b"null operand" in L.mi_last_error()
    assert call(K=33) == -22 and b"K <= 32" in L.mi_last_error()
    assert call(K=0) == -22 and call(B=0) == -22
    assert call(H=4) == -22 and b"only upsampling" in L.mi_last_error()
    assert call(wt=3) == -22 and b"weight_type" in L.mi_last_error()
    assert call(wt=-1) == -22
    assert call(eps=0.0) == -22 and b"eps" in L.mi_last_error()
    need = L.mi_upsample_gdl_workspace(2, 5, 7, 19, 20, 28)
    assert need >= 2 * 20 * 7 * 19 * 4 + 2 * 19 * 4 + (3 * 19 + 1) * 4
    assert call(nbytes=need - 1) != 0 and b"workspace too small" in L.mi_last_error()
    assert L.mi_upsample_gdl_workspace(0, 5, 7, 19, 20, 28) == 0
