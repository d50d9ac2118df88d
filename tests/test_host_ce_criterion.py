"""CPU tests of kernels.CeCriterion, the one checked value that carries the criterion of the fused upsample + cross-entropy heads (class weights,
label smoothing, OHEM, focal exponent) from the layers to kernels.upsample_ce_head: what `of` returns for every accepted combination, the exception
type and message of every refused one, and the order of the refusals (OHEM's first)."""
import pytest
import torch

from rnd_semantic_segmentation_amd import kernels

W = torch.tensor([1.0, 2.0, 0.5])
OHEM_MSG = "ohem .*cannot be combined with class_weights / label_smoothing"
FOCAL_MSG = "focal_gamma .*cannot be combined with ohem / label_smoothing"

# (keywords of `of`, the value it returns as a plain tuple)
ACCEPTED = [
    ("defaults", {}, (None, 0.0, None, 0.0)),
    ("weights", {"class_weights": W}, (W, 0.0, None, 0.0)),
    ("smoothing", {"label_smoothing": 0.1}, (None, 0.1, None, 0.0)),
    ("weights+smoothing", {"class_weights": W, "label_smoothing": 0.1}, (W, 0.1, None, 0.0)),
    ("ohem", {"ohem": (0.7, 3)}, (None, 0.0, (0.7, 3), 0.0)),
    ("focal", {"focal_gamma": 2.0}, (None, 0.0, None, 2.0)),
    ("focal+weights", {"focal_gamma": 2.0, "class_weights": W}, (W, 0.0, None, 2.0)),
]


@pytest.mark.parametrize("name,kw,want", ACCEPTED, ids=[a[0] for a in ACCEPTED])
def test_of_returns_the_checked_values(name, kw, want):
    crit = kernels.CeCriterion.of(**kw)
    assert isinstance(crit, kernels.CeCriterion)
    assert crit.class_weights is want[0]          # the tensor itself: nothing is copied or moved
    assert (crit.label_smoothing, crit.ohem, crit.focal_gamma) == want[1:]
    assert type(crit.label_smoothing) is float and type(crit.focal_gamma) is float
    assert kernels.CeCriterion.of(*want)[1:] == crit[1:]          # the positional order is the keywords' and the fields'


def test_of_converts_what_the_checks_convert():
    crit = kernels.CeCriterion.of(label_smoothing=0, ohem=[1, 10.0], focal_gamma=0)
    assert crit == (None, 0.0, (1.0, 10), 0.0)
    assert type(crit.ohem) is tuple and type(crit.ohem[0]) is float and type(crit.ohem[1]) is int
    assert kernels.CeCriterion.of(focal_gamma=8).focal_gamma == kernels.FOCAL_GAMMA_MAX
    # zero exponent and zero smoothing switch nothing on: OHEM goes with them
    assert kernels.CeCriterion.of(ohem=(0.7, 3), focal_gamma=0.0, label_smoothing=0.0).ohem == (0.7, 3)


def test_the_value_is_immutable():
    crit = kernels.CeCriterion.of(focal_gamma=2.0)
    with pytest.raises(AttributeError):
        crit.focal_gamma = 0.0
    with pytest.raises(AttributeError):
        crit.extra = 1


REFUSED = [
    ("ohem+weights", {"ohem": (0.7, 3), "class_weights": W}, NotImplementedError, OHEM_MSG),
    ("ohem+smoothing", {"ohem": (0.7, 3), "label_smoothing": 0.1}, NotImplementedError, OHEM_MSG),
    ("focal+ohem", {"focal_gamma": 2.0, "ohem": (0.7, 3)}, NotImplementedError, FOCAL_MSG),
    ("focal+smoothing", {"focal_gamma": 2.0, "label_smoothing": 0.1}, NotImplementedError, FOCAL_MSG),
    ("focal+weights+smoothing", {"focal_gamma": 0.5, "class_weights": W, "label_smoothing": 0.1}, NotImplementedError, FOCAL_MSG),
    ("gamma<0", {"focal_gamma": -1.0}, ValueError, r"focal_gamma -1.0 lies outside \[0, 8\]"),
    ("gamma>8", {"focal_gamma": 8.5}, ValueError, r"focal_gamma 8.5 lies outside \[0, 8\]"),
    ("gamma nan", {"focal_gamma": float("nan")}, ValueError, r"focal_gamma nan lies outside \[0, 8\]"),
    ("gamma text", {"focal_gamma": "much"}, ValueError, r"focal_gamma must be a number in \[0, 8\], got 'much'"),
    ("ohem not a pair", {"ohem": 0.7}, ValueError, r"ohem must be \(thresh, min_kept\), got 0.7"),
    ("ohem three", {"ohem": (0.7, 3, 1)}, ValueError, r"ohem must be \(thresh, min_kept\)"),
    ("ohem thresh", {"ohem": (1.5, 3)}, ValueError, r"ohem: thresh 1.5 lies outside \[0, 1\]"),
    ("ohem min_kept 0", {"ohem": (0.7, 0)}, ValueError, "ohem: min_kept must be an integer >= 1, got 0"),
    ("ohem min_kept 2.5", {"ohem": (0.7, 2.5)}, ValueError, "ohem: min_kept must be an integer >= 1, got 2.5"),
]


@pytest.mark.parametrize("name,kw,exc,msg", REFUSED, ids=[r[0] for r in REFUSED])
def test_of_refuses_with_the_helpers_type_and_message(name, kw, exc, msg):
    with pytest.raises(exc, match=msg) as e:
        kernels.CeCriterion.of(**kw)
    assert type(e.value) is exc


def test_the_refusals_come_in_the_pinned_order():
    """refuse_ohem_with_weights, then refuse_focal_with (the exponent's range inside it), then check_ohem."""
    with pytest.raises(NotImplementedError, match=OHEM_MSG):          # everything set: OHEM's message wins
        kernels.CeCriterion.of(class_weights=W, label_smoothing=0.1, ohem=(0.7, 3), focal_gamma=2.0)
    with pytest.raises(NotImplementedError, match=OHEM_MSG):          # ... over an exponent out of range and a malformed pair too
        kernels.CeCriterion.of(label_smoothing=0.1, ohem=(7, 0), focal_gamma=9.0)
    with pytest.raises(ValueError, match="focal_gamma 9.0 lies outside"):          # the exponent's range before the pair's form
        kernels.CeCriterion.of(ohem=(7, 0), focal_gamma=9.0)
    with pytest.raises(NotImplementedError, match=FOCAL_MSG):          # focal with OHEM before the pair's form
        kernels.CeCriterion.of(ohem=(7, 0), focal_gamma=2.0)
    with pytest.raises(ValueError, match="ohem: thresh 7.0 lies outside"):
        kernels.CeCriterion.of(ohem=(7, 0))


def test_the_helpers_stay_public_and_are_what_of_calls(monkeypatch):
    calls = []
    for name in ("refuse_ohem_with_weights", "refuse_focal_with", "check_ohem"):
        real = getattr(kernels, name)
        monkeypatch.setattr(kernels, name, lambda *a, name=name, real=real: (calls.append(name), real(*a))[1])
    kernels.CeCriterion.of(ohem=(0.7, 3))
    assert calls == ["refuse_ohem_with_weights", "refuse_focal_with", "check_ohem"]
    del calls[:]
    kernels.CeCriterion.of(class_weights=W, focal_gamma=2.0)
    assert calls == ["refuse_ohem_with_weights", "refuse_focal_with"]          # no pair, nothing to check
    assert kernels.check_focal_gamma(2) == 2.0


def test_the_layers_keep_their_keywords_and_one_constant():
    import inspect

    from rnd_semantic_segmentation_amd.host import engine, gald, modules, plugin
    four = ["class_weights", "label_smoothing", "ohem", "focal_gamma"]
    for fn in (modules.ASPP_Classifier_V2.loss, gald.GCPADecoder.losses, gald.GCPADecoder.loss, kernels.CeCriterion.of):
        params = inspect.signature(fn).parameters
        assert [p for p in params if p in four] == four, fn
        assert [params[p].default for p in four] == [None, 0.0, None, 0.0], fn
    assert list(inspect.signature(kernels.upsample_ce_head).parameters) == ["low", "labels", "crit", "want_grad", "grad_scale", "ignore_index",
                                                                            "align_corners"]
    assert list(inspect.signature(gald._GaldRun.ce_head).parameters) == ["self", "low", "labels", "ignore_index", "crit", "inv_t"]
    assert plugin.FOCAL_GAMMA_MAX is kernels.FOCAL_GAMMA_MAX
    assert not hasattr(engine, "AsppOhemLossFn") and not hasattr(engine, "AsppFocalLossFn") and not hasattr(gald.GCPADecoder, "_ce_extra")
