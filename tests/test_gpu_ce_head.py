"""GPU test of kernels.upsample_ce_head, the one entry of the fused upsample + cross-entropy heads: for every accepted kernels.CeCriterion it makes the
launch the direct wrapper makes (K.upsample_ce, K.upsample_ce_ohem, K.upsample_ce_focal) and nothing else, so loss_out and dlow carry the same bits -
at grad_scale 1 and 0.5 and loss-only.  The bar is bit equality because both are the same launch on the same operands; the bits are compared as
integers, which is torch.equal on every number and also holds where a loss is nan (no valid pixel with a weight: nan != nan as floats)."""
import functools

import pytest
import torch

import _wce_ref as R

pytestmark = pytest.mark.gpu

SHAPES = ["one", "k1", "ident", "k19_ac", "k19", "k32", "tiles"]
OHEM = (0.7, 3)          # on these sizes both branches of the threshold are hit: 0.7 itself and the 3rd smallest probability
# name -> (CeCriterion.of's keywords given the weights, the C-ABI entry the criterion has to reach)
CRITERIA = {
    "defaults": (lambda w: {}, "mi_upsample_ce_ex"),
    "weights": (lambda w: {"class_weights": w}, "mi_upsample_ce_w"),
    "smoothing": (lambda w: {"label_smoothing": 0.1}, "mi_upsample_ce_w"),
    "weights+smoothing": (lambda w: {"class_weights": w, "label_smoothing": 0.1}, "mi_upsample_ce_w"),
    "ohem": (lambda w: {"ohem": OHEM}, "mi_upsample_ce_ohem"),
    "focal": (lambda w: {"focal_gamma": 2.0}, "mi_upsample_ce_focal"),
    "focal+weights": (lambda w: {"focal_gamma": 2.0, "class_weights": w}, "mi_upsample_ce_focal"),
}
ENTRIES = ("mi_upsample_ce_ex", "mi_upsample_ce_w", "mi_upsample_ce_ohem", "mi_upsample_ce_focal")


@pytest.fixture(scope="module")
def K():
    import __graft_entry__ as entry
    entry.build()
    from rnd_semantic_segmentation_amd import kernels
    return kernels


@functools.lru_cache(maxsize=None)
def operands(name):
    """(low, labels, weights) of one tests/_wce_ref.SHAPES row on the device: made once, shared, never written to."""
    low, lab, w = R.shape_inputs(R.SHAPE_BY_NAME[name])
    return torch.from_numpy(low).cuda(), torch.from_numpy(lab).cuda(), torch.from_numpy(w).cuda()


def direct(K, low, lab, kw, **call):
    """The wrapper a layer called before there was one entry."""
    if kw.get("focal_gamma", 0.0) > 0.0:
        return K.upsample_ce_focal(low, lab, kw["focal_gamma"], class_weights=kw.get("class_weights"), **call)
    if "ohem" in kw:
        return K.upsample_ce_ohem(low, lab, kw["ohem"][0], kw["ohem"][1], **call)[:2]
    return K.upsample_ce(low, lab, class_weights=kw.get("class_weights"), label_smoothing=kw.get("label_smoothing", 0.0), **call)


def same_bits(a, b):
    return a.dtype == b.dtype == torch.float32 and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("criterion", list(CRITERIA))
@pytest.mark.parametrize("shape", SHAPES)
def test_the_head_is_the_direct_wrappers_launch(K, monkeypatch, shape, criterion):
    from rnd_semantic_segmentation_amd import _lib
    low, lab, w = operands(shape)
    make_kw, entry = CRITERIA[criterion]
    kw = make_kw(w)
    crit = K.CeCriterion.of(**kw)
    align = R.SHAPE_BY_NAME[shape].align_corners
    want = {(gs, grad): direct(K, low, lab, kw, want_grad=grad, grad_scale=gs, align_corners=align)
            for gs, grad in ((1.0, True), (0.5, True), (1.0, False))}
    reached = []
    for name in ENTRIES:
        real = getattr(_lib.lib(), name)
        monkeypatch.setattr(_lib.lib(), name, lambda *a, name=name, real=real: (reached.append(name), real(*a))[1])
    for (gs, grad), (want_out, want_d) in want.items():
        out, dlow = K.upsample_ce_head(low, lab, crit, want_grad=grad, grad_scale=gs, align_corners=align)
        torch.cuda.synchronize()
        assert same_bits(out, want_out), (shape, criterion, gs, grad, out.tolist(), want_out.tolist())
        if grad:
            assert dlow.shape == low.shape and same_bits(dlow, want_d), (shape, criterion, gs)
        else:
            assert dlow is None and want_d is None
    assert reached == [entry] * 3, reached          # one call of the C-ABI per head, through the criterion's own entry
