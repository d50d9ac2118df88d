"""GPU tests of class weights and label smoothing in the fused upsample + cross-entropy heads (mi_upsample_ce_w, csrc/upsample_ce.hip) and the layers
above it: K.upsample_ce(class_weights=, label_smoothing=) against the float64 restatement (tests/_wce_ref.py) and torch's own F.cross_entropy in
float64, the default call's bits against mi_upsample_ce_ex, edge values, properties (bit-reproducible, loss-only, graph capture with the weights read
at replay), ASPP_Classifier_V2.loss, the GALD decoder's heads, CrossEntropyNHWC, and one ASPPTrainer / GALDTrainer step with the keys set.

Bars: those of the fused upsample losses in tests/test_gpu_ops.py / test_gpu_gdl.py - loss and S 2e-5 relative, dlow 2e-5 of the expectation's
largest magnitude.  (torch's own fp32 run of "k19_ac" with weights and smoothing lies 1.1e-7 / 2.6e-7 from float64: two decades inside.)"""
import functools
import logging

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _cases
import _wce_ref as R
from rnd_semantic_segmentation_amd.host import synth

pytestmark = pytest.mark.gpu

LOSS_BAR, GRAD_BAR = 2e-5, 2e-5


@pytest.fixture(scope="module")
def K():
    import __graft_entry__ as entry
    entry.build()
    from rnd_semantic_segmentation_amd import kernels
    return kernels


def relmax(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want).max() / np.abs(want).max()


@functools.lru_cache(maxsize=None)
def shape_ref(name, variant):
    """(low, labels, weights or None, smoothing, restatement, torch float64 (loss, dlow)) of one shape and variant: computed once, shared, never written to."""
    shape = R.SHAPE_BY_NAME[name]
    _, use_w, s = [v for v in R.VARIANTS if v[0] == variant][0]
    low, lab, w = R.shape_inputs(shape)
    w = w if use_w else None
    return low, lab, w, s, R.wce_ref(low, lab, w, s, shape.align_corners), R.wce_autograd(low, lab, w, s, shape.align_corners)


def fused(K, low, lab, w, s, align_corners, want_grad=True, **kw):
    """K.upsample_ce on numpy operands -> (loss_out [4] numpy, dlow [B,h,w,K] numpy or None)."""
    out, dlow = K.upsample_ce(torch.from_numpy(low).cuda(), torch.from_numpy(lab).cuda(), want_grad=want_grad, align_corners=align_corners,
                              class_weights=None if w is None else torch.from_numpy(np.asarray(w, np.float32)).cuda(), label_smoothing=s, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), None if dlow is None else dlow.cpu().numpy()


def check_against(r, out, dlow, what):
    assert np.isfinite(out[:3]).all() and np.isfinite(dlow).all(), what
    assert out[2] == float(r.bad), (what, out)
    loss, S = float(r.loss), float(r.S)
    e_loss = abs(float(out[0]) - loss) / abs(loss) if loss != 0.0 else abs(float(out[0]))
    e_S = abs(float(out[1]) - S) / S
    dmax = float(r.dlow.abs().max())
    e_d = relmax(dlow, r.dlow.numpy()) if dmax > 0 else float(np.abs(dlow).max())
    print("%s: loss %.3e rel, S %.3e rel, dlow %.3e relmax" % (what, e_loss, e_S, e_d))
    assert e_loss < LOSS_BAR and e_S < LOSS_BAR and e_d < GRAD_BAR, (what, e_loss, e_S, e_d)


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("variant", [v[0] for v in R.VARIANTS])
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: s.name)
def test_parity_with_the_restatement_and_torch_float64(K, shape, variant):
    low, lab, w, s, r, (tloss, td) = shape_ref(shape.name, variant)
    out, dlow = fused(K, low, lab, w, s, shape.align_corners)
    check_against(r, out, dlow, "%s/%s" % (shape.name, variant))
    tl = float(tloss)
    e_loss = abs(float(out[0]) - tl) / abs(tl) if tl != 0.0 else abs(float(out[0]))
    e_d = relmax(dlow, td.numpy()) if float(td.abs().max()) > 0 else float(np.abs(dlow).max())
    print("%s/%s vs torch float64: loss %.3e rel, dlow %.3e relmax" % (shape.name, variant, e_loss, e_d))
    assert e_loss < LOSS_BAR and e_d < GRAD_BAR, (e_loss, e_d)
    if shape.K == 1:
        assert out[0] == 0.0


# ------------------------------------------------------------------------------------------------ 2. the defaults
def _raw_w(K, lowd, labd, cw, s, align_corners, want_grad=True):
    """mi_upsample_ce_w itself (K.upsample_ce does not call it at the defaults)."""
    from rnd_semantic_segmentation_amd import _lib
    B, h, w, Kc = lowd.shape
    _, H, W = labd.shape
    L = _lib.lib()
    ws = torch.empty(L.mi_upsample_ce_workspace(B, h, w, Kc, H, W), dtype=torch.uint8, device=lowd.device)
    out = torch.empty(4, dtype=torch.float32, device=lowd.device)
    dlow = torch.empty_like(lowd) if want_grad else None
    p = K._p
    _lib.check(L.mi_upsample_ce_w(p(lowd), p(labd), p(cw), p(out), p(dlow), B, h, w, Kc, H, W, 255, float(s), 1.0, int(align_corners), p(ws), ws.numel(),
                                  K._stream()), "mi_upsample_ce_w")
    torch.cuda.synchronize()
    return out, dlow


@pytest.mark.parametrize("name", ["k19_ac", "k19", "tiles_ac", "tiles", "k32"])
def test_null_weights_and_no_smoothing_give_the_bytes_of_the_plain_entry(K, name):
    shape = R.SHAPE_BY_NAME[name]
    low, lab, _ = R.shape_inputs(shape)
    lowd, labd = torch.from_numpy(low).cuda(), torch.from_numpy(lab).cuda()
    want, want_d = K.upsample_ce(lowd, labd, align_corners=shape.align_corners)
    got, got_d = _raw_w(K, lowd, labd, None, 0.0, shape.align_corners)
    assert torch.equal(got[:3], want[:3]) and torch.equal(got_d, want_d)
    lo, none = _raw_w(K, lowd, labd, None, 0.0, shape.align_corners, want_grad=False)
    assert none is None and torch.equal(lo[:3], want[:3])
    # weights of 1 go through the weighted instantiation: the same loss within the bars (the compiler contracts the two instantiations differently)
    ones, ones_d = _raw_w(K, lowd, labd, torch.ones(shape.K, device="cuda"), 0.0, shape.align_corners)
    assert abs(float(ones[0]) - float(want[0])) < LOSS_BAR * float(want[0]) and ones[1] == want[1]
    assert float((ones_d - want_d).abs().max()) < GRAD_BAR * float(want_d.abs().max())


def test_default_arguments_do_not_reach_the_new_symbol(K, monkeypatch):
    from rnd_semantic_segmentation_amd import _lib
    shape = R.SHAPE_BY_NAME["k19_ac"]
    low, lab, w = R.shape_inputs(shape)
    lowd, labd = torch.from_numpy(low).cuda(), torch.from_numpy(lab).cuda()

    def refuse(*a):
        raise AssertionError("mi_upsample_ce_w called")

    monkeypatch.setattr(_lib.lib(), "mi_upsample_ce_w", refuse)
    out, dlow = K.upsample_ce(lowd, labd)
    out2, _ = K.upsample_ce(lowd, labd, class_weights=None, label_smoothing=0.0, want_grad=False)
    torch.cuda.synchronize()
    assert torch.equal(out[:3], out2[:3]) and dlow is not None
    for kw in ({"label_smoothing": 0.1}, {"class_weights": torch.from_numpy(w).cuda()}):
        with pytest.raises(AssertionError, match="mi_upsample_ce_w called"):
            K.upsample_ce(lowd, labd, **kw)


# ------------------------------------------------------------------------------------------------ 3. edge values
def test_every_pixel_ignored_gives_nan_and_a_zero_gradient(K):
    shape = R.SHAPE_BY_NAME["k19_ac"]
    low, lab, w = R.shape_inputs(shape)
    out, dlow = fused(K, low, np.full_like(lab, 255), w, 0.1, True)
    assert np.isnan(out[0]) and out[1] == 0.0 and out[2] == 0.0
    assert np.isfinite(dlow).all() and not dlow.any()          # torch leaves the gradient of ignored pixels at zero
    # the identity scale, where a dlow row IS a pixel: the ignored pixels' rows are exactly zero beside valid ones
    ident = R.SHAPE_BY_NAME["ident"]
    low2, lab2, w2 = R.shape_inputs(ident)
    lab2 = np.full_like(lab2, int(np.flatnonzero(w2 > 0)[0]))
    lab2[0, 0, 1] = 255
    out2, dlow2 = fused(K, low2, lab2, w2, 0.1, False)
    assert np.isfinite(out2[0]) and not dlow2[0, 0, 1].any() and dlow2[0, 1, 0].any()
    check_against(R.wce_ref(low2, lab2, w2, 0.1, False), out2, dlow2, "identity with an ignored pixel")


def test_only_a_zero_weight_class_gives_nan(K):
    shape = R.SHAPE_BY_NAME["k19_ac"]
    low, lab, w = R.shape_inputs(shape)
    zero = int(np.flatnonzero(w == 0)[0])
    out, _ = fused(K, low, np.full_like(lab, zero), w, 0.0, True)
    assert np.isnan(out[0]) and out[1] == 0.0
    assert np.isnan(float(R.wce_autograd(low, np.full_like(lab, zero), w, 0.0, True)[0]))          # torch: nan too


def test_out_of_range_labels_are_left_out_and_counted(K):
    shape = R.SHAPE_BY_NAME["k19_ac"]
    low, lab, w = R.shape_inputs(shape)
    bad = lab.copy()
    bad.reshape(-1)[[3, 500, 501, 2000, 2969]] = [19, 254, -1, 1000, 2 ** 40]
    r = R.wce_ref(low, bad, w, 0.1, True)
    assert r.bad == 5
    out, dlow = fused(K, low, bad, w, 0.1, True)
    assert out[2] == 5.0
    check_against(r, out, dlow, "five bad labels")
    as_ignored = bad.copy()
    as_ignored[(bad < 0) | (bad >= 19)] = 255
    same, same_d = fused(K, low, as_ignored, w, 0.1, True)
    assert same[:2].tobytes() == out[:2].tobytes() and same_d.tobytes() == dlow.tobytes() and same[2] == 0.0
    from rnd_semantic_segmentation_amd import kernels
    with pytest.raises(ValueError, match="5 label values"):
        kernels.check_labels(torch.from_numpy(out), 19)


def test_logits_of_magnitude_80_stay_finite_with_smoothing(K):
    """A confidently wrong pixel: log p_c is formed as (z_c - max) - log(sum exp), so nothing underflows into log(0)."""
    shape = R.SHAPE_BY_NAME["k19_ac"]
    low, lab = R.make_inputs("wce.sat", shape.B, shape.K, shape.hw, shape.HW, magnitude=80.0)
    w = R.make_weights("wce.sat", shape.K)
    assert np.abs(low).max() == np.float32(80.0)
    r = R.wce_ref(low, lab, w, 0.1, True)
    assert float(r.loss) > 10.0
    out, dlow = fused(K, low, lab, w, 0.1, True)
    check_against(r, out, dlow, "magnitude 80")


# ------------------------------------------------------------------------------------------------ 4. properties
def test_two_calls_are_bit_equal_and_loss_only_gives_the_same_bits(K):
    for name in ("k19", "tiles_ac", "f32"):
        shape = R.SHAPE_BY_NAME[name]
        low, lab, w, s, _, _ = shape_ref(name, "ws")
        a, b = fused(K, low, lab, w, s, shape.align_corners), fused(K, low, lab, w, s, shape.align_corners)
        assert a[0][:3].tobytes() == b[0][:3].tobytes() and a[1].tobytes() == b[1].tobytes()
        out, dlow = fused(K, low, lab, w, s, shape.align_corners, want_grad=False)
        assert dlow is None and out[:3].tobytes() == a[0][:3].tobytes()


def test_the_call_is_capturable_and_a_replay_reads_the_weights_anew(K):
    shape = R.SHAPE_BY_NAME["k19"]
    low, lab, w, s, r, _ = shape_ref("k19", "ws")
    lowd, labd = torch.from_numpy(low).cuda(), torch.from_numpy(lab).cuda()
    wd = torch.ones(shape.K, device="cuda")
    K.upsample_ce(lowd, labd, align_corners=False, class_weights=wd, label_smoothing=s)          # outside the capture: code objects, LDS attribute
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, dlow = K.upsample_ce(lowd, labd, align_corners=False, class_weights=wd, label_smoothing=s)
    graph.replay()
    torch.cuda.synchronize()
    ones_out, ones_d = K.upsample_ce(lowd, labd, align_corners=False, class_weights=torch.ones(shape.K, device="cuda"), label_smoothing=s)
    torch.cuda.synchronize()
    assert torch.equal(out[:3], ones_out[:3]) and torch.equal(dlow, ones_d)
    wd.copy_(torch.from_numpy(w))          # in place: the captured pointer, new values
    graph.replay()
    torch.cuda.synchronize()
    eager_out, eager_d = K.upsample_ce(lowd, labd, align_corners=False, class_weights=torch.from_numpy(w).cuda(), label_smoothing=s)
    torch.cuda.synchronize()
    assert torch.equal(out[:3], eager_out[:3]) and torch.equal(dlow, eager_d) and not torch.equal(out[:2], ones_out[:2])
    check_against(r, out.cpu().numpy(), dlow.cpu().numpy(), "graph replay with the new weights")


# ------------------------------------------------------------------------------------------------ 5. layers
def _tiny_aspp():
    from rnd_semantic_segmentation_amd.host import modules
    fe = modules.resnet_feature_extractor("resnet101", freeze_bn=True, pretrained_backbone=False, layers=(1, 1, 2, 2))
    cls = modules.ASPP_Classifier_V2(2048, [6, 12, 18, 24], [6, 12, 18, 24], 19)
    for m in (fe, cls):
        synth.load_formula_weights(m)
        m.cuda()
        m.ensure_flat()
    return fe, cls


def test_aspp_classifier_loss_with_weights_smoothing_and_temperature(K):
    """ASPP_Classifier_V2.loss (C = 2048 head on the 17 x 17 feature of the tiny backbone at 129 x 129) with class weights, smoothing 0.1 and temperature
    1.8 against F.cross_entropy on the classifier's own materialised forward(x, size) / 1.8: the loss, and the gradient that reaches the head's bias."""
    T = 1.8
    x, lab = _cases.net_inputs(2, 129, 71)
    labd = torch.from_numpy(lab).cuda().long()
    w = torch.from_numpy(R.make_weights("wce.aspp", 19)).cuda()
    fe, cls = _tiny_aspp()
    with torch.no_grad():
        feat = fe(torch.from_numpy(x).cuda()).detach()
    assert tuple(feat.shape[-2:]) == (17, 17)
    loss = cls.loss(feat, labd, 255, temperature=T, class_weights=w, label_smoothing=0.1)
    loss.backward()
    torch.cuda.synchronize()
    got_b = dict(cls.named_parameters())["conv2d_list.0.bias"].grad.detach().clone()
    plain = _tiny_aspp()[1].loss(feat, labd, 255, temperature=T)
    _, ref_cls = _tiny_aspp()
    out = ref_cls(feat, (129, 129)).float()
    want = F.cross_entropy(out / T, labd, weight=w, ignore_index=255, label_smoothing=0.1)
    want.backward()
    torch.cuda.synchronize()
    want_b = dict(ref_cls.named_parameters())["conv2d_list.0.bias"].grad.detach()
    e_loss, e_b = abs(float(loss) - float(want)) / float(want), relmax(got_b.cpu().numpy(), want_b.cpu().numpy())
    print("ASPP head: loss %.6f (plain %.6f), %.3e rel; bias gradient %.3e relmax" % (float(loss), float(plain), e_loss, e_b))
    assert e_loss < LOSS_BAR and e_b < GRAD_BAR, (e_loss, e_b)
    assert float(loss) != float(plain)


def _gald_inputs():
    x = torch.from_numpy(synth.synth_image(2, 224, 224, seed=5)).cuda()
    lab = torch.from_numpy(synth.synth_label(2, 224, 224, 19, seed=5)).long().cuda()
    return x, lab


def test_decoder_heads_with_weights_and_smoothing_match_the_restatement_on_their_own_logits(K):
    """GCPAEncoder + GCPADecoder, 2 x 3 x 224 x 224, criterion="ce" with class weights and smoothing: each of the four losses equals the restatement on
    the tapped low-resolution logits (linear5 .. linear2), and after backward each head's bias gradient equals the restatement's dlow summed over
    B, h, w and weighted 0.4 / 0.6 / 0.8 / 1 (fp32 on the tape, as in test_gpu_gdl.py)."""
    from rnd_semantic_segmentation_amd.host import gald
    x, lab = _gald_inputs()
    w = R.make_weights("wce.gald", 19)
    torch.manual_seed(3)
    enc, dec = gald.GCPAEncoder().cuda().train(), gald.GCPADecoder().cuda().train()
    with torch.no_grad():
        dec.long_relation.gamma.fill_(0.3)
    dec._taps = {}
    ls = dec.losses(x, enc(x), lab, criterion="ce", class_weights=torch.from_numpy(w).cuda(), label_smoothing=0.1)
    (ls[3] * 1 + ls[2] * 0.8 + ls[1] * 0.6 + ls[0] * 0.4).backward()
    torch.cuda.synchronize()
    assert dec.__dict__.get("bad_labels") is not None and float(dec.bad_labels) == 0.0
    labn = lab.cpu().numpy()
    for loss, i, weight in zip(ls, (5, 4, 3, 2), (0.4, 0.6, 0.8, 1.0)):
        low = dec._taps["linear%d" % i].t.detach().cpu().numpy()
        r = R.wce_ref(low, labn, w, 0.1, False)
        e_loss = abs(float(loss) - float(r.loss)) / float(r.loss)
        want = r.dlow.sum((0, 1, 2)).numpy() * weight
        e_b = relmax(getattr(dec, "linear%d" % i).bias.grad.cpu().numpy(), want)
        print("linear%d: loss %.6f, %.3e rel; bias gradient %.3e relmax" % (i, float(loss), e_loss, e_b))
        assert e_loss < LOSS_BAR and e_b < GRAD_BAR, (i, e_loss, e_b)


def test_cross_entropy_nhwc_with_weight_and_smoothing_against_torch(K):
    from rnd_semantic_segmentation_amd.host import gald
    g = torch.Generator().manual_seed(7)
    logits = (torch.randn(2, 19, 37, 53, generator=g) * 2).cuda()
    lab = torch.randint(0, 19, (2, 37, 53), generator=g)
    lab[torch.rand(2, 37, 53, generator=g) < 0.2] = 255
    lab = lab.cuda()
    w = torch.from_numpy(R.make_weights("wce.nhwc", 19))
    crit = gald.CrossEntropyNHWC(ignore_index=255, weight=w, label_smoothing=0.1).cuda()
    a = logits.clone().requires_grad_(True)
    loss = crit(a, lab)
    loss.backward()
    b = logits.double().cpu().requires_grad_(True)
    want = F.cross_entropy(b, lab.cpu(), weight=w.double(), ignore_index=255, label_smoothing=0.1)
    want.backward()
    e_loss, e_d = abs(float(loss) - float(want)) / float(want), relmax(a.grad.cpu().numpy(), b.grad.numpy())
    print("CrossEntropyNHWC: loss %.3e rel, gradient %.3e relmax" % (e_loss, e_d))
    assert e_loss < LOSS_BAR and e_d < GRAD_BAR
    plain = gald.CrossEntropyNHWC(ignore_index=255)(logits, lab)          # the default call: gk.gce, as before
    assert abs(float(plain) - float(F.cross_entropy(logits.double().cpu(), lab.cpu(), ignore_index=255))) < LOSS_BAR * float(plain)


def _cfg(tmp_path, *opts):
    from rnd_semantic_segmentation_amd.host import config as hc
    cfg = hc.CfgNode(hc.default_tree())
    cfg.merge_from_list(["OUTPUT_DIR", str(tmp_path), "MODEL.NUM_CLASSES", 19, "MODEL.FREEZE_BN", True, "SOLVER.EPOCHS", 1, "SOLVER.BASE_LR", 1e-4] + list(opts))
    cfg.freeze()
    return cfg


WEIGHTED = ["SOLVER.LABEL_SMOOTHING", 0.1, "SOLVER.CLASS_WEIGHTS", str(tuple(float(v) for v in R.make_weights("wce.trainer", 19)))]


def test_aspp_trainer_step_with_the_keys_set_and_at_their_defaults(K, tmp_path):
    from rnd_semantic_segmentation_amd.host import modules
    from rnd_semantic_segmentation_amd.host.trainer import ASPPTrainer

    class Tiny(ASPPTrainer):
        build_feature_extractor = staticmethod(lambda cfg: modules.resnet_feature_extractor("resnet101", freeze_bn=True, pretrained_backbone=False,
                                                                                            layers=(1, 1, 2, 2)))

    x, lab = _cases.net_inputs(2, 65, 11)
    xt, lt = torch.from_numpy(x), torch.from_numpy(lab)

    def make(*opts):
        tr = Tiny("aspp", _cfg(tmp_path, *opts), [None] * 50, 0, logger=logging.getLogger("wce-aspp"))
        with torch.no_grad():
            for m in (tr.feature_extractor, tr.classifier):
                synth.load_formula_weights(m)
                m._store.generation += 1
        return tr

    tr = make(*WEIGHTED)
    assert tr.ce_weights.is_cuda and tr.ce_weights.shape == (19,) and tr.ce_smoothing == 0.1
    before = tr.classifier._store.data.clone()
    loss, _ = tr.train_step(xt, lt, 40)
    plain = make()
    assert plain.ce_kwargs == {}
    loss0, _ = plain.train_step(xt, lt, 40)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss)) and not torch.equal(before, tr.classifier._store.data)
    assert float(loss) != float(loss0)
    # the defaults: the loss bits of this tree's default path
    other = make()
    want = other.classifier.loss(other.feature_extractor(xt.cuda()), lt.cuda().long(), 255)
    torch.cuda.synchronize()
    assert torch.equal(loss0, want.detach())
    # the weighted step is classifier.loss with the helper's tensors
    again = make(*WEIGHTED)
    want_w = again.classifier.loss(again.feature_extractor(xt.cuda()), lt.cuda().long(), 255, class_weights=again.ce_weights, label_smoothing=0.1)
    torch.cuda.synchronize()
    assert torch.equal(loss, want_w.detach())


def test_gald_trainer_step_with_the_keys_set_and_at_their_defaults(K, tmp_path):
    from rnd_semantic_segmentation_amd.host import gald
    x, lab = _gald_inputs()

    def make(*opts):
        log = logging.getLogger("wce-gald")
        log.addHandler(logging.NullHandler())
        torch.manual_seed(11)
        tr = gald.GALDTrainer("gald", _cfg(tmp_path, *opts), None, 0, logger=log)
        tr.encoder.train()
        tr.decoder.train()
        return tr

    tr = make(*WEIGHTED)
    assert tr.criterion.weight is tr.ce_weights or torch.equal(tr.criterion.weight, tr.ce_weights)
    before = tr.decoder._store.data.clone()
    loss, _ = tr.train_step(x, lab, 100)
    plain = make()
    loss0, _ = plain.train_step(x, lab, 100)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss)) and not torch.equal(before, tr.decoder._store.data)
    assert gald.take_bad_labels(tr.decoder, tr.criterion) == 0
    assert float(loss) != float(loss0)
    other = make()
    l5, l4, l3, l2 = other.decoder.losses(x, other.encoder(x), lab, criterion="ce")
    want = l2 * 1 + l3 * 0.8 + l4 * 0.6 + l5 * 0.4
    torch.cuda.synchronize()
    assert torch.equal(loss0, want.detach())
